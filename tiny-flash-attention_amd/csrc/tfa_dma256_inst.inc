// tfa_dma256_inst.inc — the LDS-DMA kernel 256 wide for one dtype: the partial pass of tfa_fwd_splitkv at head dims 136..256
// (fp32 partial O + LSE per key chunk, the chunk index in the grid).  Compiled as the units tfa_dma_inst_<dtype>_256.
#include "tfa_launch.h"

namespace tfa {

template <typename T, bool CAUSAL, bool NT>
static hipError_t launch_splitkv_wide_one(const KArgs& a, hipStream_t stream, LaunchGeom* geom, bool dry) {
  constexpr int D = 256, NW = 4, VF = VF_PAIR | VF_2BUF | (NT ? VF_DMA_NT : 0);
  constexpr int lds = 4 * 64 * D * 2;                          // two K and two V tile buffers
  auto kern = fwd_kernel_dma<T, D, NW, CAUSAL, true, VF>;
  const int nitems = a.nbh * a.nwork * (a.nsplit > 1 ? a.nsplit : 1);
  static std::atomic<unsigned long long> attr_mask{0};         // one per instantiation, one bit per device
  return launch_common(kern, attr_mask, nitems, NW * 64, lds, a, stream, geom, dry);
}

template <>
hipError_t launch_splitkv_wide<TFA_T>(const KArgs& a, bool causal, hipStream_t s, LaunchGeom* g, bool dry) {
  if (a.nsplit > 1 && a.kv_stream && a.nmb == 1 && a.H == a.Hk)      // decode over a large K/V cache: non-temporal K/V loads
    return causal ? launch_splitkv_wide_one<TFA_T, true, true>(a, s, g, dry) : launch_splitkv_wide_one<TFA_T, false, true>(a, s, g, dry);
  return causal ? launch_splitkv_wide_one<TFA_T, true, false>(a, s, g, dry) : launch_splitkv_wide_one<TFA_T, false, false>(a, s, g, dry);
}

}  // namespace tfa
