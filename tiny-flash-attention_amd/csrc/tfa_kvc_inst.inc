// tfa_kvc_inst.inc — instantiates one form of the KV-cache kernel (tfa_fwd_kernel_dma.h: fwd_kernel_dma_kvc; tfa_launch.h: TFA_KVC_FORMS) for one (TFA_T, TFA_D):
// causal and not, fp32 partials (split) with and without the non-temporal hint, and the 16-bit direct output of a single chunk.  Compiled as the units
// tfa_<kvc|kvc8>_inst[_win|_tree][_pack][_vq[_sched]]_<dtype>_<W>: every word of the name is one define below (Makefile: W_<word>).
#include "tfa_launch.h"
#include "tfa_kvcache.h"
#ifndef TFA_KVC_FP8
#define TFA_KVC_FP8 0        // 1: the e4m3 cache (tfa_kvc8_inst_*) — Kvc8Args in KvcArgs' place; T is the type of q and out
#endif
#ifndef TFA_KVC_PACK
#define TFA_KVC_PACK 0       // 1: the packed form (*_pack_*) — KvcPacked<> of the cache side's struct
#endif
#ifndef TFA_KVC_VQ
#define TFA_KVC_VQ 0         // 1: the varlen-q form (*_vq_*) — KvcVarlenQ<> behind that
#endif
#ifndef TFA_KVC_SCHED
#define TFA_KVC_SCHED 0      // 1 (with TFA_KVC_VQ): the scheduled form (*_vq_sched_*) — KvcSched<> behind that
#endif
#ifndef TFA_KVC_WIN
#define TFA_KVC_WIN 0        // 1 (with any of the above): the form's windowed form (*_inst_win_*) — KvcWindow<> behind them all: the causal template only, the 16-bit
#endif                       // direct output and the fp32 partials, no non-temporal twin
#ifndef TFA_KVC_TREE
#define TFA_KVC_TREE 0       // 1 (with any of the forms, not with TFA_KVC_WIN): the form's tree form (*_inst_tree_*) — KvcTree<> behind them all: the causal template only,
#endif                       // the 16-bit direct output and the fp32 partials, no non-temporal twin
#if TFA_KVC_TREE && TFA_KVC_WIN
#error "the tree form has no windowed form"
#endif
#if TFA_KVC_SCHED && !TFA_KVC_VQ
#error "the scheduled form is a form of the varlen-q form"
#endif

namespace tfa {

// the arguments of this unit's kernels
using UnitArgs = KvcForm<TFA_KVC_FP8 != 0, TFA_KVC_PACK != 0, TFA_KVC_SCHED ? KVC_SCHED : TFA_KVC_VQ ? KVC_VQ : KVC_PLAIN,
                         TFA_KVC_WIN ? KVC_WIN : TFA_KVC_TREE ? KVC_TREE : KVC_NONE>::Args;

template <typename T, int D, bool CAUSAL, bool F32OUT, bool NT>
static hipError_t launch_kvc_one(const UnitArgs& a_in, hipStream_t stream, LaunchGeom* geom, bool dry) {
  constexpr int lds = 4 * 64 * D * 2;                          // two K and two V tile buffers
#if TFA_KVC_WIN
  static_assert(CAUSAL && !NT, "the windowed form: causal, no non-temporal twin");
#elif TFA_KVC_TREE
  static_assert(CAUSAL && !NT, "the tree form: causal, no non-temporal twin");
#endif
  auto kern = fwd_kernel_dma_kvc<T, D, CAUSAL, F32OUT, NT, UnitArgs>;
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

template <>
hipError_t launch_kvc<TFA_T, TFA_D, UnitArgs>(const UnitArgs& a, bool causal, bool f32out, bool nt, hipStream_t s, LaunchGeom* g, bool dry) {
#if TFA_KVC_WIN || TFA_KVC_TREE
  if (!causal || nt) return hipErrorInvalidValue;
  return f32out ? launch_kvc_one<TFA_T, TFA_D, true, true, false>(a, s, g, dry) : launch_kvc_one<TFA_T, TFA_D, true, false, false>(a, s, g, dry);
#else
  if (!f32out) return causal ? launch_kvc_one<TFA_T, TFA_D, true, false, false>(a, s, g, dry) : launch_kvc_one<TFA_T, TFA_D, false, false, false>(a, s, g, dry);
  if (nt) return causal ? launch_kvc_one<TFA_T, TFA_D, true, true, true>(a, s, g, dry) : launch_kvc_one<TFA_T, TFA_D, false, true, true>(a, s, g, dry);
  return causal ? launch_kvc_one<TFA_T, TFA_D, true, true, false>(a, s, g, dry) : launch_kvc_one<TFA_T, TFA_D, false, true, false>(a, s, g, dry);
#endif
}

}  // namespace tfa
