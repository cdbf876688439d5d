// tfa_kvc8_inst.inc — instantiates the e4m3 form of the KV-cache kernel (tfa_fwd_kernel_dma.h: fwd_kernel_dma_kvc8) for one (TFA_T, TFA_D), as tfa_kvc_inst.inc does for
// the 16-bit form: causal and not, fp32 partials (split) with and without the non-temporal hint, the 16-bit direct output of a single chunk.  Compiled as the units tfa_kvc8_inst_<dtype>_<W>.
#include "tfa_launch.h"
#include "tfa_kvcache.h"
#ifndef TFA_KVC_PACK
#define TFA_KVC_PACK 0       // 1: the unit of the packed form (tfa_kvc8_inst_pack_<dtype>_<W>) — the same launchers over fwd_kernel_dma_kvc8_pack and its arguments
#endif
#ifndef TFA_KVC_VQ
#define TFA_KVC_VQ 0         // 1: the unit of the varlen-q form (tfa_kvc8_inst_vq_<dtype>_<W>, tfa_kvc8_inst_pack_vq_<dtype>_<W>) — the same launchers over fwd_kernel_dma_kvc_vq
#endif
#ifndef TFA_KVC_SCHED
#define TFA_KVC_SCHED 0      // 1 (with TFA_KVC_VQ): the unit of the scheduled form (tfa_kvc8_inst_vq_sched_<dtype>_<W>, tfa_kvc8_inst_pack_vq_sched_<dtype>_<W>) — fwd_kernel_dma_kvc_vq over KvcSched<>
#endif
#ifndef TFA_KVC_WIN
#define TFA_KVC_WIN 0        // 1 (with any of the above): the unit of the form's windowed form (tfa_kvc8_inst_win_*) — fwd_kernel_dma_kvc_win over KvcWindow<> of the form's arguments:
#endif                       // the causal template only, the 16-bit direct output and the fp32 partials, no non-temporal twin
#ifndef TFA_KVC_TREE
#define TFA_KVC_TREE 0       // 1 (with any of the forms, not with TFA_KVC_WIN): the unit of the form's tree form (tfa_kvc8_inst_tree_*) — fwd_kernel_dma_kvc_tree over KvcTree<> of the
#endif                       // form's arguments: the causal template only, the 16-bit direct output and the fp32 partials, no non-temporal twin
#if TFA_KVC_TREE && TFA_KVC_WIN
#error "the tree form has no windowed form"
#endif
#if TFA_KVC_SCHED && !TFA_KVC_VQ
#error "the scheduled form is a form of the varlen-q form"
#endif

namespace tfa {

// the arguments of this unit's kernels: the form's struct, behind it the packed form's (TFA_KVC_PACK), behind both the varlen-q form's (TFA_KVC_VQ)
using UnitBase = std::conditional_t<TFA_KVC_PACK != 0, KvcPacked<Kvc8Args>, Kvc8Args>;
using UnitVq = std::conditional_t<TFA_KVC_VQ != 0, KvcVarlenQ<UnitBase>, UnitBase>;
using UnitForm = std::conditional_t<TFA_KVC_SCHED != 0, KvcSched<UnitVq>, UnitVq>;     // ... and behind the three the scheduled form's (TFA_KVC_SCHED)
using UnitWin = std::conditional_t<TFA_KVC_WIN != 0, KvcWindow<UnitForm>, UnitForm>;   // ... and behind them all the window's (TFA_KVC_WIN)
using UnitArgs = std::conditional_t<TFA_KVC_TREE != 0, KvcTree<UnitWin>, UnitWin>;     // ... or the tree's (TFA_KVC_TREE)

template <typename T, int D, bool CAUSAL, bool F32OUT, bool NT>
static hipError_t launch_kvc8_one(const UnitArgs& a_in, hipStream_t stream, LaunchGeom* geom, bool dry) {
  constexpr int lds = 4 * 64 * D * 2;                          // two K and two V tile buffers of DECODED (16-bit) tiles: the 16-bit form's size
#if TFA_KVC_WIN
  static_assert(CAUSAL && !NT, "the windowed form: causal, no non-temporal twin");
  auto kern = fwd_kernel_dma_kvc_win<T, D, F32OUT, UnitArgs>;
#elif TFA_KVC_TREE
  static_assert(CAUSAL && !NT, "the tree form: causal, no non-temporal twin");
  auto kern = fwd_kernel_dma_kvc_tree<T, D, F32OUT, UnitArgs>;
#elif TFA_KVC_VQ
  auto kern = fwd_kernel_dma_kvc_vq<T, D, CAUSAL, F32OUT, NT, UnitArgs>;
#elif TFA_KVC_PACK
  auto kern = fwd_kernel_dma_kvc8_pack<T, D, CAUSAL, F32OUT, NT>;
#else
  auto kern = fwd_kernel_dma_kvc8<T, D, CAUSAL, F32OUT, NT>;
#endif
  const int grid = a_in.nbh * a_in.nwork * (a_in.nsplit > 1 ? a_in.nsplit : 1);
  if (geom) { geom->grid = grid; geom->block = 256; geom->lds = lds; }
  if (dry) return hipSuccess;
  auto a = a_in;
  fill_decode(&a);
  static std::atomic<unsigned long long> attr_mask{0};         // one per instantiation, one bit per device
  hipError_t e = set_dyn_lds_once(attr_mask, reinterpret_cast<const void*>(kern), lds);
  if (e != hipSuccess) return e;
  (void)hipGetLastError();
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, stream, a);
  return hipGetLastError();
}

#if TFA_KVC_WIN
template <>
hipError_t launch_kvc_win<TFA_T, TFA_D, UnitArgs>(const UnitArgs& a, bool f32out, hipStream_t s, LaunchGeom* g, bool dry) {
  return f32out ? launch_kvc8_one<TFA_T, TFA_D, true, true, false>(a, s, g, dry) : launch_kvc8_one<TFA_T, TFA_D, true, false, false>(a, s, g, dry);
}
#elif TFA_KVC_TREE
template <>
hipError_t launch_kvc_tree<TFA_T, TFA_D, UnitArgs>(const UnitArgs& a, bool f32out, hipStream_t s, LaunchGeom* g, bool dry) {
  return f32out ? launch_kvc8_one<TFA_T, TFA_D, true, true, false>(a, s, g, dry) : launch_kvc8_one<TFA_T, TFA_D, true, false, false>(a, s, g, dry);
}
#else
template <>
#if TFA_KVC_VQ
hipError_t launch_kvc_vq<TFA_T, TFA_D, UnitArgs>(const UnitArgs& a,
#elif TFA_KVC_PACK
hipError_t launch_kvc8_pack<TFA_T, TFA_D>(const KvcPacked<Kvc8Args>& a,
#else
hipError_t launch_kvc8<TFA_T, TFA_D>(const Kvc8Args& a,
#endif
                                        bool causal, bool f32out, bool nt, hipStream_t s, LaunchGeom* g, bool dry) {
  if (!f32out) return causal ? launch_kvc8_one<TFA_T, TFA_D, true, false, false>(a, s, g, dry) : launch_kvc8_one<TFA_T, TFA_D, false, false, false>(a, s, g, dry);
  if (nt) return causal ? launch_kvc8_one<TFA_T, TFA_D, true, true, true>(a, s, g, dry) : launch_kvc8_one<TFA_T, TFA_D, false, true, true>(a, s, g, dry);
  return causal ? launch_kvc8_one<TFA_T, TFA_D, true, true, false>(a, s, g, dry) : launch_kvc8_one<TFA_T, TFA_D, false, true, false>(a, s, g, dry);
}
#endif

}  // namespace tfa
