// tfa_bwd_inst.inc — instantiates the backward kernels for one (dtype, head dim); compiled as the units tfa_bwd_inst_* (the Makefile turns a unit's name into the defines)
#include <hip/hip_runtime.h>
#include "tfa_bwd_launch.h"

namespace tfa {

template <typename T, int D, int MODE, bool CAUSAL, bool F32OUT, int DVB = D / 32>
static hipError_t launch_bwd_one(const BArgs& a, int grid, hipStream_t stream, bool dry) {
  constexpr bool WIDE256 = D > 128;                // one wave per SIMD, unified images (tfa_bwd_kernel.h)
  constexpr int NW = WIDE256 ? 4 : 8;
  constexpr int lds = bwd_lds_bytes<D, MODE, WIDE256>();   // two stages of tile images (+ the stages' row statistics, dK / dV): tfa_bwd_launch.h
  constexpr bool CAN_BIG = WIDE256 ? DVB == D / 32 : MODE == BWD_DQ;   // (256 wide: all three modes, in the unit of the full column count)
  if (a.big && !CAN_BIG) return hipErrorInvalidValue;       // (the host never asks: tfa_bwd_api.hip)
  auto kern = bwd_kernel<T, D, MODE, CAUSAL, F32OUT, WIDE256, NW, false, DVB>;
  if constexpr (CAN_BIG) {                                   // (only the forms that can be asked for are instantiated)
    if (a.big) {
      static std::atomic<unsigned long long> attr_mask_big{0};
      return launch_bwd_kernel(bwd_kernel<T, D, MODE, CAUSAL, F32OUT, WIDE256, NW, true>, attr_mask_big, grid, NW * 64, lds, a, stream, dry);
    }
  }
  static std::atomic<unsigned long long> attr_mask{0};   // one per instantiation, one bit per device (tfa_launch.h)
  return launch_bwd_kernel(kern, attr_mask, grid, NW * 64, lds, a, stream, dry);
}

template <typename T, int D, int MODE, int DVB = D / 32>
static hipError_t launch_bwd_mode(const BArgs& a, int grid, bool causal, bool f32out, hipStream_t s, bool dry) {
  if (causal) return f32out ? launch_bwd_one<T, D, MODE, true, true, DVB>(a, grid, s, dry) : launch_bwd_one<T, D, MODE, true, false, DVB>(a, grid, s, dry);
  return f32out ? launch_bwd_one<T, D, MODE, false, true, DVB>(a, grid, s, dry) : launch_bwd_one<T, D, MODE, false, false, DVB>(a, grid, s, dry);
}

#if defined(TFA_DVB)
// one unit per (dtype, valid column blocks) of the 256-wide kernels: tfa_bwd_inst_<dtype>_256_v<5..8>
template <>
hipError_t launch_bwd_wide<TFA_T, TFA_DVB>(const BArgs& a, int mode, int grid, bool causal, bool f32out, hipStream_t s, bool dry) {
  switch (mode) {
    case BWD_DQ: return launch_bwd_mode<TFA_T, 256, BWD_DQ, TFA_DVB>(a, grid, causal, f32out, s, dry);
    case BWD_DK: return launch_bwd_mode<TFA_T, 256, BWD_DK, TFA_DVB>(a, grid, causal, f32out, s, dry);
    default: return launch_bwd_mode<TFA_T, 256, BWD_DV, TFA_DVB>(a, grid, causal, f32out, s, dry);
  }
}
#elif TFA_D == 256
template <> hipError_t launch_bwd_wide<TFA_T, 5>(const BArgs&, int, int, bool, bool, hipStream_t, bool);
template <> hipError_t launch_bwd_wide<TFA_T, 6>(const BArgs&, int, int, bool, bool, hipStream_t, bool);
template <> hipError_t launch_bwd_wide<TFA_T, 7>(const BArgs&, int, int, bool, bool, hipStream_t, bool);
template <> hipError_t launch_bwd_wide<TFA_T, 8>(const BArgs&, int, int, bool, bool, hipStream_t, bool);
// head dims 136..256: the unit of the valid-column-block count does the work (only the columns that can hold data are multiplied)
template <>
hipError_t launch_bwd<TFA_T, TFA_D>(const BArgs& a, int mode, int grid, bool causal, bool f32out, hipStream_t s, bool dry) {
  if (a.big) return launch_bwd_wide<TFA_T, 8>(a, mode, grid, causal, f32out, s, dry);   // slices of 2 GiB and more: the windowed instantiations exist for all eight column blocks only
  switch ((a.dv + 31) / 32) {
    case 5: return launch_bwd_wide<TFA_T, 5>(a, mode, grid, causal, f32out, s, dry);
    case 6: return launch_bwd_wide<TFA_T, 6>(a, mode, grid, causal, f32out, s, dry);
    case 7: return launch_bwd_wide<TFA_T, 7>(a, mode, grid, causal, f32out, s, dry);
    default: return launch_bwd_wide<TFA_T, 8>(a, mode, grid, causal, f32out, s, dry);
  }
}
#else
template <>
hipError_t launch_bwd<TFA_T, TFA_D>(const BArgs& a, int mode, int grid, bool causal, bool f32out, hipStream_t s, bool dry) {
  // head dims that leave the last 32-column block empty (up to 96 in the 128-wide kernel, up to 32 in the 64-wide one): the dQ launch
  // multiplies the valid blocks only (the fused dK/dV launch below does the same)
  if (mode == BWD_DQ && !a.big && a.dv <= TFA_D - 32) return launch_bwd_mode<TFA_T, TFA_D, BWD_DQ, TFA_D / 32 - 1>(a, grid, causal, f32out, s, dry);
  switch (mode) {
    case BWD_DQ: return launch_bwd_mode<TFA_T, TFA_D, BWD_DQ>(a, grid, causal, f32out, s, dry);
    case BWD_DK: return launch_bwd_mode<TFA_T, TFA_D, BWD_DK>(a, grid, causal, f32out, s, dry);
    default: return launch_bwd_mode<TFA_T, TFA_D, BWD_DV>(a, grid, causal, f32out, s, dry);
  }
}
#endif

#if !defined(TFA_DVB) && TFA_D <= 128   // the fused dK/dV launch and the workspace dQ exist 64 and 128 wide (head dims above 128: three single-gradient launches)
template <typename T, int D, bool CAUSAL, bool F32OUT, bool WS>
static hipError_t launch_bwd_kv_one(const BArgs& a, int grid, hipStream_t stream, bool dry) {
  constexpr int KG = TFA_BWD_KV_KG_OF(WS);
  constexpr int lds = bwd_kv_lds_bytes<D, KG>();   // three stages of (Q, dO) tiles + the P exchange buffers + the stages' row statistics: tfa_bwd_launch.h
  if constexpr (!WS) {
    if (!a.big && a.dv <= D - 32) {                  // the last 32-column block is empty: the instantiation that skips it
      static std::atomic<unsigned long long> attr_mask_n{0};
      return launch_bwd_kernel(bwd_kv_kernel<T, D, CAUSAL, F32OUT, false, KG, false, D / 32 - 1>, attr_mask_n, grid, KG * 128, lds, a, stream, dry);
    }
  }
  auto kern = bwd_kv_kernel<T, D, CAUSAL, F32OUT, WS, KG>;
  auto kern_big = bwd_kv_kernel<T, D, CAUSAL, F32OUT, false, TFA_BWD_KV_KG_OF(false), true>;
  if (a.big && WS) return hipErrorInvalidValue;
  if (a.big) {
    static std::atomic<unsigned long long> attr_mask_big{0};
    return launch_bwd_kernel(kern_big, attr_mask_big, grid, KG * 128, lds, a, stream, dry);
  }
  static std::atomic<unsigned long long> attr_mask{0};
  return launch_bwd_kernel(kern, attr_mask, grid, KG * 128, lds, a, stream, dry);
}

template <>
hipError_t launch_bwd_kv<TFA_T, TFA_D>(const BArgs& a, int grid, bool causal, bool f32out, hipStream_t s, bool dry) {
  if (a.ws) {
    if (causal) return f32out ? launch_bwd_kv_one<TFA_T, TFA_D, true, true, true>(a, grid, s, dry) : launch_bwd_kv_one<TFA_T, TFA_D, true, false, true>(a, grid, s, dry);
    return f32out ? launch_bwd_kv_one<TFA_T, TFA_D, false, true, true>(a, grid, s, dry) : launch_bwd_kv_one<TFA_T, TFA_D, false, false, true>(a, grid, s, dry);
  }
  if (causal) return f32out ? launch_bwd_kv_one<TFA_T, TFA_D, true, true, false>(a, grid, s, dry) : launch_bwd_kv_one<TFA_T, TFA_D, true, false, false>(a, grid, s, dry);
  return f32out ? launch_bwd_kv_one<TFA_T, TFA_D, false, true, false>(a, grid, s, dry) : launch_bwd_kv_one<TFA_T, TFA_D, false, false, false>(a, grid, s, dry);
}

template <typename T, int D, bool CAUSAL, bool F32OUT>
static hipError_t launch_bwd_dq_ws_one(const BArgs& a, int grid, hipStream_t stream, bool dry) {
  constexpr int lds = 3 * (64 * 256 * 2 + 64 * D * 2);               // three stages of (dS^T tile, K tile)
  static std::atomic<unsigned long long> attr_mask{0};
  return launch_bwd_kernel(bwd_dq_ws_kernel<T, D, CAUSAL, F32OUT>, attr_mask, grid, 512, lds, a, stream, dry);
}

template <>
hipError_t launch_bwd_dq_ws<TFA_T, TFA_D>(const BArgs& a, int grid, bool causal, bool f32out, hipStream_t s, bool dry) {
  if (causal) return f32out ? launch_bwd_dq_ws_one<TFA_T, TFA_D, true, true>(a, grid, s, dry) : launch_bwd_dq_ws_one<TFA_T, TFA_D, true, false>(a, grid, s, dry);
  return f32out ? launch_bwd_dq_ws_one<TFA_T, TFA_D, false, true>(a, grid, s, dry) : launch_bwd_dq_ws_one<TFA_T, TFA_D, false, false>(a, grid, s, dry);
}

#endif

#if !defined(TFA_DVB)
template <>
hipError_t launch_delta<TFA_T, TFA_D>(const void* o, const void* dout, float* delta, const long long* os, const long long* ds, int H, int Nq,
                                      long long rows, int dv, hipStream_t s, bool dry) {
  if (dry) return hipSuccess;
  constexpr int LPR = TFA_D / 8;
  const long long threads = rows * LPR;
  const int grid = (int)((threads + 255) / 256);
  (void)hipGetLastError();
  hipLaunchKernelGGL((bwd_delta_kernel<TFA_T, TFA_D>), dim3(grid), dim3(256), 0, s, o, dout, delta, os[0], os[1], os[2], ds[0], ds[1], ds[2], H, Nq, rows, dv);
  return hipGetLastError();
}
#endif

}  // namespace tfa
