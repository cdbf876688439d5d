// tfa_bwd_launch.h — host-side declarations shared by the backward instantiation units and tfa_bwd_api.hip
#pragma once
#include <hip/hip_runtime.h>
#include "tfa_bwd_kernel.h"
#include "tfa_bwd_kv_kernel.h"
#include "tfa_bwd_dq_kernel.h"
#include "tfa_host_util.h"

// key groups (32 resident keys each) per workgroup of the fused dK/dV kernel: 4 (eight waves, two per SIMD, 186 registers, no
// scratch — the default) or 6 (twelve waves, three per SIMD at 168 registers with 15-18 of them spilled: 1-3 % faster in one
// measurement, 15 % SLOWER in the next build of the same kernel code once other scratch-using kernels shared the library —
// profiles/r03_bwd_kg_ab.txt; a kernel that touches scratch is at the mercy of the runtime's scratch sizing, so it stays an arm:
// -DTFA_BWD_KV_KG=6).  The workspace form is blocked by 128 keys and always uses 4.
#ifndef TFA_BWD_KV_KG
#define TFA_BWD_KV_KG 4
#endif
#define TFA_BWD_KV_KG_OF(WS) ((WS) ? 4 : TFA_BWD_KV_KG)

namespace tfa {
// dynamic LDS of the backward kernels — ONE formula per kernel for every launcher (fixed-length: tfa_bwd_inst.inc, the varlen and local forms:
// tfa_bwd_form_inst.inc).  bwd_kernel: two stages of NIMG tile images, plus the stages' row statistics in the key-resident (dK / dV) modes.
template <int D, int MODE, bool WIDE256>
constexpr int bwd_lds_bytes() {
  return 2 * ((WIDE256 || MODE == BWD_DV) ? 2 : 3) * 64 * D * 2 + (MODE == BWD_DQ ? 0 : 2 * 512);
}
// bwd_kv_kernel: three stages of (Q, dO) tiles, the P exchange buffers (bwd_kv_kernel: NPX), the stages' row statistics
template <int D, int KG>
constexpr int bwd_kv_lds_bytes() {
  return 3 * 2 * 64 * D * 2 + (KG == 4 ? 3 : 2) * KG * (32 * 64 * 2) + 3 * 512;
}
// the common tail of every launcher of a BArgs kernel (the counterpart of tfa_launch.h: launch_common): nothing on a dry run; else opt in to the dynamic
// LDS size on this device, launch, and return THIS launch's status (a sticky error left behind by unrelated earlier HIP calls is cleared first)
template <typename Kern>
static inline hipError_t launch_bwd_kernel(Kern kern, std::atomic<unsigned long long>& mask, int grid, int block, int lds, const BArgs& a, hipStream_t stream,
                                           bool dry) {
  if (dry) return hipSuccess;
  hipError_t e = set_dyn_lds_once(mask, reinterpret_cast<const void*>(kern), lds);
  if (e != hipSuccess) return e;
  (void)hipGetLastError();
  hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, stream, a);
  return hipGetLastError();
}

template <typename T, int D>
hipError_t launch_bwd(const BArgs& a, int mode, int grid, bool causal, bool f32out, hipStream_t stream, bool dry);
// the 256-wide single-gradient kernels by the number of 32-column blocks that can hold valid head-dim columns (5..8)
template <typename T, int DVB>
hipError_t launch_bwd_wide(const BArgs& a, int mode, int grid, bool causal, bool f32out, hipStream_t stream, bool dry);
// dK and dV in one launch (tfa_bwd_kv_kernel.h): grid = B * Hk * ceil(Nk / 128)
template <typename T, int D>
hipError_t launch_bwd_kv(const BArgs& a, int grid, bool causal, bool f32out, hipStream_t stream, bool dry);   // a.ws != nullptr: also writes dS
// dQ = scale * dS . K from the workspace (tfa_bwd_dq_kernel.h): grid = B * H * ceil(Nq / 256)
template <typename T, int D>
hipError_t launch_bwd_dq_ws(const BArgs& a, int grid, bool causal, bool f32out, hipStream_t stream, bool dry);
// the forms of the two-launch backward (tfa_host_util.h: TFA_FORMS_BWD — packed variable-length, local, and the local kernels' ALiBi, softcap and (fixed-length only) dense-bias forms): keys = false
// the dQ launch (grid = B * H * ceil(Nq / 256)), keys = true the fused dK/dV launch (grid = B * Hk * ceil(Nk / 128)) — Nq / Nk = max_seqlen_q / _k for varlen.
// The local kernels are the causal template only (`causal` is ignored).  One unit per (dtype, width, form): tfa_bwd_inst_varlen_<dtype>_<D> and
// tfa_bwd_inst_<local|alibi|softcap>_<dtype>_<D>_<fx|vl>, each specialising launch_bwd_form (tfa_bwd_form_inst.inc)
template <typename T, int D, int FORM>
hipError_t launch_bwd_form(const BArgs& a, bool keys, int grid, bool causal, bool f32out, hipStream_t stream, bool dry);
#define TFA_BWD_FORM_UNIT(T, D, FORM) template <> hipError_t launch_bwd_form<T, D, (FORM)>(const BArgs&, bool, int, bool, bool, hipStream_t, bool);
#define TFA_BWD_FORM_UNITS(FORM) TFA_FORM_SHAPES(TFA_BWD_FORM_UNIT, FORM)
TFA_FORMS_BWD(TFA_BWD_FORM_UNITS)
#undef TFA_BWD_FORM_UNITS
#undef TFA_BWD_FORM_UNIT
template <typename T, int D>
hipError_t launch_delta(const void* o, const void* dout, float* delta, const long long* os, const long long* ds, int H, int Nq, long long rows,
                        int dv, hipStream_t stream, bool dry);
}  // namespace tfa
