// tfa_fwd_inst.inc — instantiates the kernel variants for one (TFA_T, TFA_D, TFA_CAUSAL).
// Compiled as the units tfa_fwd_inst_<dtype>_<D>_c<0|1> so the eight units compile in parallel.
// Product build: the dispatched kernels only; -DTFA_EXPERIMENTAL adds the A/B arms (tfa_launch.h).
#include "tfa_launch.h"

namespace tfa {

// (the unit's causal flavour only: `causal` is TFA_CAUSAL wherever this expands)
#define TFA_CF_DISPATCH(FN, ...)                                                           \
  (void)causal;                                                                            \
  return f32out ? FN<__VA_ARGS__, TFA_CAUSAL, true>(a, s, g, dry) : FN<__VA_ARGS__, TFA_CAUSAL, false>(a, s, g, dry);

template <typename T, int D, int NW, int VF, bool CAUSAL, bool F32OUT>
static hipError_t launch_one_dma(const KArgs& a, hipStream_t stream, LaunchGeom* geom, bool dry) {
  constexpr int lds = ((VF & VF_2BUF) ? 4 : 6) * 64 * D * 2;   // K and V tile buffers
  auto kern = fwd_kernel_dma<T, D, NW, CAUSAL, F32OUT, VF>;
  const int nitems = a.nbh * a.nwork * (a.nsplit > 1 ? a.nsplit : 1);
  // persistent: one workgroup per CU slot (LDS admits one 8-wave or one 4-wave workgroup of this kernel per CU)
  int grid = nitems;
  if ((VF & VF_PERSIST) && a.grid > 0 && a.grid * ((VF & VF_2BUF) ? 2 : 1) < nitems) grid = a.grid * ((VF & VF_2BUF) ? 2 : 1);
  static std::atomic<unsigned long long> attr_mask{0};   // one per instantiation, one bit per device
  return launch_common(kern, attr_mask, grid, NW * 64, lds, a, stream, geom, dry);
}
template <typename T, int D, int NW, int VF>
static hipError_t launch_dma(const KArgs& a, bool causal, bool f32out, hipStream_t s, LaunchGeom* g, bool dry) {
  TFA_CF_DISPATCH(launch_one_dma, T, D, NW, VF)
}

template <typename T, int D, int NW, int VF>
static hipError_t launch_il(const KArgs& a, bool causal, bool f32out, hipStream_t s, LaunchGeom* g, bool dry) {
  TFA_CF_DISPATCH(launch_one_il, T, D, NW, VF)
}
// The main instantiation of a product kernel has a twin that writes the cycle stamps of tfa_debug_set_trace (ILAB_TRACE, tfa_fwd_kernel_il.h); the
// special-case instantiations (windowed, idle-wave, narrow) leave a trace buffer untouched.  16-bit output only (the tools trace bf16 problems).
template <typename T, int D, int NW, int VF>
static hipError_t launch_il_main(const KArgs& a, bool causal, bool f32out, hipStream_t s, LaunchGeom* g, bool dry) {
  if (a.trace != nullptr && !f32out) return launch_one_il<T, D, NW, VF, TFA_CAUSAL, false, D / 32, ILAB_TRACE>(a, s, g, dry);
  return launch_il<T, D, NW, VF>(a, causal, f32out, s, g, dry);
}
// the two main kernels also exist with the last 32-column block left out (head dims up to 96 / up to 32: tfa_fwd_kernel_il.h, DVB)
template <typename T, int D, int NW, int VF>
static hipError_t launch_il_narrow(const KArgs& a, bool causal, bool f32out, hipStream_t s, LaunchGeom* g, bool dry) {
  (void)causal;
  return f32out ? launch_one_il<T, D, NW, VF, TFA_CAUSAL, true, D / 32 - 1>(a, s, g, dry) : launch_one_il<T, D, NW, VF, TFA_CAUSAL, false, D / 32 - 1>(a, s, g, dry);
}

#if defined(TFA_EXPERIMENTAL)
template <typename T, int D, int NW, int VF, int RB, bool CAUSAL, bool F32OUT>
static hipError_t launch_one(const KArgs& a, hipStream_t stream, LaunchGeom* geom, bool dry) {
  constexpr int lds = 4 * 64 * D * 2;   // K0 K1 V0 V1
  auto kern = fwd_kernel<T, D, NW, CAUSAL, F32OUT, VF, 0, RB>;
  static std::atomic<unsigned long long> attr_mask{0};
  return launch_common(kern, attr_mask, a.nbh * a.nwork, NW * 64, lds, a, stream, geom, dry);
}
template <typename T, int D, int NW, int VF, int RB = 1>
static hipError_t launch_cf(const KArgs& a, bool causal, bool f32out, hipStream_t s, LaunchGeom* g, bool dry) {
  TFA_CF_DISPATCH(launch_one, T, D, NW, VF, RB)
}

template <typename T, int D, int VF, bool CAUSAL, bool F32OUT>
static hipError_t launch_one_pp(const KArgs& a, hipStream_t stream, LaunchGeom* geom, bool dry) {
  constexpr int lds = 4 * 64 * D * 2;
  auto kern = fwd_kernel_pp<T, D, CAUSAL, F32OUT, VF>;
  static std::atomic<unsigned long long> attr_mask{0};
  return launch_common(kern, attr_mask, a.nbh * a.nwork, 512, lds, a, stream, geom, dry);
}
template <typename T, int D, int VF>
static hipError_t launch_pp(const KArgs& a, bool causal, bool f32out, hipStream_t s, LaunchGeom* g, bool dry) {
  TFA_CF_DISPATCH(launch_one_pp, T, D, VF)
}

template <typename T, int D, int VF, bool CAUSAL, bool F32OUT>
static hipError_t launch_one_swp(const KArgs& a, hipStream_t stream, LaunchGeom* geom, bool dry) {
  constexpr int lds = 6 * 64 * D * 2;
  auto kern = fwd_kernel_swp<T, D, CAUSAL, F32OUT, VF>;
  static std::atomic<unsigned long long> attr_mask{0};
  return launch_common(kern, attr_mask, a.nbh * a.nwork, 512, lds, a, stream, geom, dry);
}
template <typename T, int D, int VF>
static hipError_t launch_swp(const KArgs& a, bool causal, bool f32out, hipStream_t s, LaunchGeom* g, bool dry) {
  TFA_CF_DISPATCH(launch_one_swp, T, D, VF)
}

template <typename T, int D, int VF, bool CAUSAL, bool F32OUT>
static hipError_t launch_one_w64(const KArgs& a, hipStream_t stream, LaunchGeom* geom, bool dry) {
  constexpr int lds = 6 * 64 * D * 2;
  auto kern = fwd_kernel_w64<T, D, CAUSAL, F32OUT, VF>;
  static std::atomic<unsigned long long> attr_mask{0};
  return launch_common(kern, attr_mask, a.nbh * a.nwork, 256, lds, a, stream, geom, dry);
}
template <typename T, int D, int VF>
static hipError_t launch_w64(const KArgs& a, bool causal, bool f32out, hipStream_t s, LaunchGeom* g, bool dry) {
  TFA_CF_DISPATCH(launch_one_w64, T, D, VF)
}
#endif   // TFA_EXPERIMENTAL

#if defined(TFA_ABLATE) && defined(TFA_EXPERIMENTAL)
// timing-only ablations of the dma8-pair kernel (bf16, D=128, bf16 out): variant = 100 + mask
template <bool CAUSAL, int AB>
static hipError_t launch_ab(const KArgs& a, hipStream_t stream, LaunchGeom* geom, bool dry) {
  constexpr int lds = 6 * 64 * TFA_D * 2;
  constexpr int VF = VF_PAIR;
  auto kern = fwd_kernel_dma<TFA_T, TFA_D, 8, CAUSAL, false, VF, AB>;
  const int grid = a.nbh * a.nwork;
  static std::atomic<unsigned long long> attr_mask{0};
  return launch_common(kern, attr_mask, grid, 512, lds, a, stream, geom, dry);
}
#define TFA_AB_CASE(M) case 100 + (M): return launch_ab<false, (M)>(a, s, g, dry);
template <int AB>
static hipError_t launch_ab64(const KArgs& a, hipStream_t stream, LaunchGeom* geom, bool dry) {
  constexpr int lds = 6 * 64 * TFA_D * 2;
  auto kern = fwd_kernel_w64<TFA_T, TFA_D, false, false, VF_PAIR, AB>;
  const int grid = a.nbh * a.nwork;
  static std::atomic<unsigned long long> attr_mask{0};
  return launch_common(kern, attr_mask, grid, 256, lds, a, stream, geom, dry);
}
#define TFA_AB64_CASE(M) case 700 + (M): return launch_ab64<(M)>(a, s, g, dry);
template <int VF, int AB>
static hipError_t launch_abil(const KArgs& a, hipStream_t stream, LaunchGeom* geom, bool dry) {
  constexpr int lds = 4 * 64 * TFA_D * 2;
  auto kern = fwd_kernel_il<TFA_T, TFA_D, 8, false, false, VF, AB>;
  const int grid = a.nbh * a.nwork;
  static std::atomic<unsigned long long> attr_mask{0};
  return launch_common(kern, attr_mask, grid, 512, lds, a, stream, geom, dry);
}
#define TFA_ABIL_CASE(M) case 1000 + (M): return launch_abil<VF_PAIR, (M)>(a, s, g, dry); case 2000 + (M): return launch_abil<VF_PAIR | VF_IL_DMASPREAD, (M)>(a, s, g, dry);
#endif

template <>
hipError_t launch_fwd_c<TFA_T, TFA_D, TFA_CAUSAL>(const KArgs& a, bool f32out, int variant, hipStream_t s, LaunchGeom* g, bool dry) {
  constexpr bool causal = TFA_CAUSAL;
  switch (variant) {
    case 17: return (a.nsplit > 1 && a.kv_stream && a.nmb == 1 && a.H == a.Hk)           // decode over a large K/V cache: non-temporal K/V loads
                        ? launch_dma<TFA_T, TFA_D, 4, VF_PAIR | VF_2BUF | VF_DMA_NT>(a, causal, f32out, s, g, dry)
                        : launch_dma<TFA_T, TFA_D, 4, VF_PAIR | VF_2BUF>(a, causal, f32out, s, g, dry);
    // (one query block with whole waves behind the last row — decode: the instantiation whose idle waves skip the tile work)
    case 30: switch (il_instantiation(30, a.big, a.Nq, a.row_mod, a.dv, TFA_D)) {
        case IL_WINDOWED: return launch_il<TFA_T, TFA_D, 8, VF_PAIR | VF_IL_DMASPREAD | VF_IL_EPI | VF_IL_WINDOWED>(a, causal, f32out, s, g, dry);
        case IL_IDLE: return launch_il<TFA_T, TFA_D, 8, VF_PAIR | VF_IL_DMASPREAD | VF_IL_EPI | VF_IL_IDLE>(a, causal, f32out, s, g, dry);
        case IL_NARROW: return launch_il_narrow<TFA_T, TFA_D, 8, VF_PAIR | VF_IL_DMASPREAD | VF_IL_EPI | VF_IL_PREF2 | VF_IL_QLDS>(a, causal, f32out, s, g, dry);
        default: return launch_il_main<TFA_T, TFA_D, 8, VF_PAIR | VF_IL_DMASPREAD | VF_IL_EPI | VF_IL_PREF2 | VF_IL_QLDS>(a, causal, f32out, s, g, dry);
      }
    case 32: switch (il_instantiation(32, a.big, a.Nq, a.row_mod, a.dv, TFA_D)) {
        case IL_WINDOWED: return launch_il<TFA_T, TFA_D, 4, VF_PAIR | VF_IL_EPI | VF_IL_EPI_INPLACE | VF_IL_WINDOWED>(a, causal, f32out, s, g, dry);
        case IL_IDLE: return launch_il<TFA_T, TFA_D, 4, VF_PAIR | VF_IL_EPI | VF_IL_EPI_INPLACE | VF_IL_IDLE>(a, causal, f32out, s, g, dry);
        case IL_NARROW: return launch_il_narrow<TFA_T, TFA_D, 4, VF_PAIR | VF_IL_EPI | VF_IL_EPI_INPLACE>(a, causal, f32out, s, g, dry);
        default: return launch_il_main<TFA_T, TFA_D, 4, VF_PAIR | VF_IL_EPI | VF_IL_EPI_INPLACE>(a, causal, f32out, s, g, dry);
      }
    case 36: return il_instantiation(36, a.big, a.Nq, a.row_mod, a.dv, TFA_D) == IL_IDLE
                        ? launch_il<TFA_T, TFA_D, 8, VF_IL_DMASPREAD | VF_IL_EPI | VF_IL_EPI_INPLACE | VF_IL_KSPLIT | VF_IL_IDLE>(a, causal, f32out, s, g, dry)
                        : launch_il_main<TFA_T, TFA_D, 8, VF_IL_DMASPREAD | VF_IL_EPI | VF_IL_EPI_INPLACE | VF_IL_KSPLIT>(a, causal, f32out, s, g, dry);
    case 37: return il_instantiation(37, a.big, a.Nq, a.row_mod, a.dv, TFA_D) == IL_IDLE
                        ? launch_il<TFA_T, TFA_D, 8, VF_PAIR | VF_IL_DMASPREAD | VF_IL_EPI | VF_IL_EPI_INPLACE | VF_IL_KSPLIT | VF_IL_IDLE>(a, causal, f32out, s, g, dry)
                        : launch_il_main<TFA_T, TFA_D, 8, VF_PAIR | VF_IL_DMASPREAD | VF_IL_EPI | VF_IL_EPI_INPLACE | VF_IL_KSPLIT>(a, causal, f32out, s, g, dry);
    // TFA_FWD_EXACT_MAX on grids the default would give to variant 30: the same kernel with the exact running maximum (slices below 2 GiB)
    case 38: return launch_il<TFA_T, TFA_D, 8, VF_PAIR | VF_IL_DMASPREAD | VF_IL_EPI | VF_IL_PREF2 | VF_IL_QLDS | VF_IL_EXACT>(a, causal, f32out, s, g, dry);
#if defined(TFA_EXPERIMENTAL)
    case 33: return launch_x4_unit<TFA_T, TFA_D>(a, causal, f32out, 0, s, g, dry);   // its own translation unit: tfa_x4_inst.inc (D <= 128: the round-2 experiment of DESIGN.md 2d)
    case 0: return launch_cf<TFA_T, TFA_D, 8, 0>(a, causal, f32out, s, g, dry);
    case 1: return launch_cf<TFA_T, TFA_D, 8, VF_TRREAD>(a, causal, f32out, s, g, dry);
    case 2: return launch_cf<TFA_T, TFA_D, 4, VF_TRREAD>(a, causal, f32out, s, g, dry);
    case 3: return launch_cf<TFA_T, TFA_D, 8, VF_TRREAD | VF_NOSKIP>(a, causal, f32out, s, g, dry);
    case 4: return launch_cf<TFA_T, TFA_D, 8, VF_TRREAD | VF_PAIR>(a, causal, f32out, s, g, dry);
    case 5: return launch_cf<TFA_T, TFA_D, 8, VF_TRREAD | VF_PAIR | VF_KPRE | VF_VPRE>(a, causal, f32out, s, g, dry);
    case 6: return launch_cf<TFA_T, TFA_D, 4, VF_TRREAD | VF_PAIR | VF_KPRE | VF_VPRE>(a, causal, f32out, s, g, dry);
    case 7: return launch_cf<TFA_T, TFA_D, 8, VF_TRREAD | VF_PAIR | VF_VPRE>(a, causal, f32out, s, g, dry);
    case 8: return launch_pp<TFA_T, TFA_D, VF_PAIR | (0 << VF_VPRE_SHIFT)>(a, causal, f32out, s, g, dry);
    case 9: return launch_pp<TFA_T, TFA_D, VF_PAIR | (2 << VF_VPRE_SHIFT)>(a, causal, f32out, s, g, dry);
    case 10: return launch_pp<TFA_T, TFA_D, VF_PAIR | (4 << VF_VPRE_SHIFT)>(a, causal, f32out, s, g, dry);
    case 11: return launch_dma<TFA_T, TFA_D, 8, VF_PAIR>(a, causal, f32out, s, g, dry);
    case 12: return launch_dma<TFA_T, TFA_D, 4, VF_PAIR>(a, causal, f32out, s, g, dry);
    case 13: return launch_dma<TFA_T, TFA_D, 8, VF_PAIR | VF_PRIO>(a, causal, f32out, s, g, dry);
    case 14: return launch_swp<TFA_T, TFA_D, VF_PAIR>(a, causal, f32out, s, g, dry);
    case 15: return launch_dma<TFA_T, TFA_D, 8, VF_PAIR | VF_PERSIST>(a, causal, f32out, s, g, dry);
    case 16: return launch_dma<TFA_T, TFA_D, 4, VF_PAIR | VF_PERSIST>(a, causal, f32out, s, g, dry);
    case 18: return launch_dma<TFA_T, TFA_D, 4, VF_PAIR | VF_2BUF | VF_PERSIST>(a, causal, f32out, s, g, dry);
    case 19: return launch_dma<TFA_T, TFA_D, 8, VF_PAIR | VF_2BUF>(a, causal, f32out, s, g, dry);
    case 20: return launch_w64<TFA_T, TFA_D, VF_PAIR>(a, causal, f32out, s, g, dry);
    case 21: return launch_dma<TFA_T, TFA_D, 4, VF_PAIR | VF_2BUF | VF_LDSEPI>(a, causal, f32out, s, g, dry);
    case 22: return launch_dma<TFA_T, TFA_D, 8, VF_PAIR | VF_2BUF | VF_LDSEPI>(a, causal, f32out, s, g, dry);
    case 23: return launch_pp<TFA_T, TFA_D, VF_PAIR | (4 << VF_VPRE_SHIFT) | (8 << VF_NOPQK_SHIFT)>(a, causal, f32out, s, g, dry);
    case 24: return launch_pp<TFA_T, TFA_D, VF_PAIR | (4 << VF_VPRE_SHIFT) | (8 << VF_NOPQK_SHIFT) | (8 << VF_NOPPV_SHIFT)>(a, causal, f32out, s, g, dry);
    case 25: return launch_pp<TFA_T, TFA_D, VF_PAIR | (4 << VF_VPRE_SHIFT) | (16 << VF_NOPQK_SHIFT)>(a, causal, f32out, s, g, dry);
    case 26: return launch_il<TFA_T, TFA_D, 8, VF_PAIR>(a, causal, f32out, s, g, dry);
    case 27: return launch_il<TFA_T, TFA_D, 4, VF_PAIR>(a, causal, f32out, s, g, dry);
    case 28: return launch_il<TFA_T, TFA_D, 8, VF_PAIR | VF_IL_DMASPREAD>(a, causal, f32out, s, g, dry);
    case 29: return launch_il<TFA_T, TFA_D, 8, VF_PAIR | VF_IL_DMASPREAD | VF_IL_DMASTAGGER>(a, causal, f32out, s, g, dry);
    case 31: return launch_il<TFA_T, TFA_D, 8, VF_PAIR | VF_IL_DMASPREAD | VF_IL_EPI | VF_IL_PREF>(a, causal, f32out, s, g, dry);
    case 35: return launch_il<TFA_T, TFA_D, 8, VF_PAIR | VF_IL_DMASPREAD | VF_IL_EPI | VF_IL_SEAM>(a, causal, f32out, s, g, dry);
#endif
#if defined(TFA_ABLATE) && defined(TFA_EXPERIMENTAL)
    TFA_AB_CASE(0) TFA_AB_CASE(1) TFA_AB_CASE(2) TFA_AB_CASE(3) TFA_AB_CASE(8) TFA_AB_CASE(16) TFA_AB_CASE(32)
    TFA_AB_CASE(48) TFA_AB_CASE(64) TFA_AB_CASE(3 + 8) TFA_AB_CASE(48 + 8) TFA_AB_CASE(48 + 64)
    TFA_AB_CASE(3 + 48 + 64) TFA_AB_CASE(8 + 48 + 64) TFA_AB_CASE(256) TFA_AB_CASE(256 + 64) TFA_AB_CASE(256 + 8 + 48 + 64) TFA_AB_CASE(3 + 8 + 48)
    TFA_ABIL_CASE(0) TFA_ABIL_CASE(1) TFA_ABIL_CASE(2) TFA_ABIL_CASE(4) TFA_ABIL_CASE(8) TFA_ABIL_CASE(9) TFA_ABIL_CASE(16 + 64) TFA_ABIL_CASE(32 + 128)
    TFA_ABIL_CASE(1 + 8 + 2) TFA_ABIL_CASE(1 + 8 + 2 + 4) TFA_ABIL_CASE(2 + 4) TFA_ABIL_CASE(64 + 128) TFA_ABIL_CASE(1 + 8 + 64 + 128) TFA_ABIL_CASE(1 + 2 + 4 + 8 + 64 + 128)
    TFA_ABIL_CASE(16 + 32 + 64 + 128) TFA_ABIL_CASE(16 + 32 + 64 + 128 + 2 + 4)
    TFA_AB64_CASE(0) TFA_AB64_CASE(1) TFA_AB64_CASE(2) TFA_AB64_CASE(4) TFA_AB64_CASE(8) TFA_AB64_CASE(9) TFA_AB64_CASE(6) TFA_AB64_CASE(15)
#endif
    default: break;
  }
#if defined(TFA_X4_ABLATE)
  if (variant >= 3000 && variant < 3256) return launch_x4_unit<TFA_T, TFA_D>(a, false, false, variant - 3000, s, g, dry);   // tools/ablate_x4.py
#endif
  return hipErrorInvalidValue;
}

}  // namespace tfa
