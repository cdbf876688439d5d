// tfa_host_util.h — host-side helpers shared by the forward and backward launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <initializer_list>
#include <stdint.h>

#include "tfa.h"

namespace tfa {

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per DEVICE: one bit per device ordinal in the launcher's mask, so a
// process that drives several GPUs opts every one of them in (devices >= 64 are simply set on every launch).
static inline hipError_t set_dyn_lds_once(std::atomic<unsigned long long>& mask, const void* kern, int lds) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const bool cacheable = dev >= 0 && dev < 64;
  const unsigned long long bit = cacheable ? (1ull << dev) : 0ull;
  if (cacheable && (mask.load(std::memory_order_acquire) & bit)) return hipSuccess;
  e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e != hipSuccess) return e;
  if (cacheable) mask.fetch_or(bit, std::memory_order_release);
  return hipSuccess;
}

// Multiprocessor count of the CURRENT device (cached per device ordinal; 256 = MI355X when no device is visible, which
// is the dry-run planning case on a CPU box).
static inline int num_cus_current_device() {
  static std::atomic<int> cache[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  const bool cacheable = dev >= 0 && dev < 64;
  if (cacheable) { const int c = cache[dev].load(std::memory_order_relaxed); if (c > 0) return c; }
  int n = 0;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return 256;
  if (cacheable) cache[dev].store(n, std::memory_order_relaxed);
  return n;
}

// A workspace size as the *_workspace entry points answer it: the product of non-negative counts, or TFA_ERR_SHAPE when it does not fit a long long (sizes
// near INT32_MAX in every dimension) — never a wrapped, negative or otherwise meaningless number.
static inline long long size_product(std::initializer_list<long long> f) {
  long long r = 1;
  for (long long x : f)
    if (x < 0 || __builtin_mul_overflow(r, x, &r)) return TFA_ERR_SHAPE;
  return r;
}

// a * b for non-negative counts, INT64_MAX when it does not fit: grids and byte counts that are only compared with a threshold
static inline long long sat_mul(long long a, long long b) {
  long long r;
  return __builtin_mul_overflow(a, b, &r) ? INT64_MAX : r;
}
// (rows * stride + d) * es in 64 bit, INT64_MAX when it does not fit: strides near INT64_MAX / 2 are arguments a caller can pass — they are refused by
// their size, never by an overflow on the way to the comparison
static inline int64_t span_bytes(int64_t rows, int64_t stride, int64_t d, int64_t es) {
  int64_t r;
  if (__builtin_mul_overflow(rows, stride, &r) || __builtin_add_overflow(r, d, &r) || __builtin_mul_overflow(r, es, &r)) return INT64_MAX;
  return r;
}

// The kernel shape a launch instantiates: element type T, compiled head-dim width W.
template <typename T_, int W_>
struct Shape {
  using T = T_;
  static constexpr int W = W_;
};
// The one dtype x width switch of the API units: calls f(Shape<T, W>{}) with T = __bf16 for TFA_BF16 and _Float16 otherwise, and W the narrowest
// of the caller's widths (ascending) that holds D — the last one when none does.  Every call site shares f's return type.
template <int W, int... Ws, typename F>
static inline auto by_dtype_width(int dtype, int D, F&& f) {
  if constexpr (sizeof...(Ws) > 0)
    if (D > W) return by_dtype_width<Ws...>(dtype, D, f);
  return dtype == TFA_BF16 ? f(Shape<__bf16, W>{}) : f(Shape<_Float16, W>{});
}

// The form of an il8 / il4 forward or backward dQ / dK/dV launch beyond the plain fixed-length one: a mask of these bits, a template argument of launch_fwd_form
// and launch_bwd_form.  The ALiBi and softcap kernels are forms of the local ones; softcap's slopes are a run-time choice of its one kernel (no ALIBI bit);
// the local kernels exist as the causal template only (the window carries the right edge).  FORM_PAGED (tfa_fwd_varlen_paged: K/V through a block table) is a
// form of the plain varlen forward alone: no window, no slopes, no cap, no backward.  FORM_BIAS (tfa_fwd_bias / tfa_bwd_bias: a dense additive bias read from
// memory inside the tile loop) is a form of the fixed-length local kernels alone: no varlen, no slopes, no cap.
enum : int { FORM_VARLEN = 1, FORM_LOCAL = 2, FORM_ALIBI = 4, FORM_SOFTCAP = 8, FORM_PAGED = 16, FORM_BIAS = 32 };
constexpr bool form_legal(int form, bool causal = true) {
  return form > 0 && form < 64 && ((form & FORM_LOCAL) ? causal : !(form & (FORM_ALIBI | FORM_SOFTCAP))) && !((form & FORM_ALIBI) && (form & FORM_SOFTCAP)) &&
         (!(form & FORM_PAGED) || form == (FORM_VARLEN | FORM_PAGED)) && (!(form & FORM_BIAS) || form == (FORM_LOCAL | FORM_BIAS));
}
// THE list of the legal forms, X(mask): each is one instantiation unit per (dtype, width) of the forward (tfa_fwd_inst_<varlen|local|alibi|softcap>_...) and of
// the backward (tfa_bwd_inst_...), fixed-length (_fx) or varlen (_vl) — the Makefile's words of those names carry the same masks.  The declarations of tfa_launch.h
// and tfa_bwd_launch.h and by_form's switch come from here.  TFA_FORMS_BWD: the forms that have a backward (by_form's, which both directions share);
// TFA_FORMS: every form — those and the forward-only paged varlen form (units tfa_fwd_inst_paged_..., reached by run_form without by_form)
#define TFA_FORMS_BWD(X)                                                                                                    \
  X(FORM_VARLEN) X(FORM_LOCAL) X(FORM_LOCAL | FORM_VARLEN) X(FORM_LOCAL | FORM_ALIBI) X(FORM_LOCAL | FORM_ALIBI | FORM_VARLEN) \
  X(FORM_LOCAL | FORM_SOFTCAP) X(FORM_LOCAL | FORM_SOFTCAP | FORM_VARLEN) X(FORM_LOCAL | FORM_BIAS)
#define TFA_FORMS(X) TFA_FORMS_BWD(X) X(FORM_VARLEN | FORM_PAGED)
// ... and the (dtype, width) pairs each of them is built for: X(T, D, ...)
#define TFA_FORM_SHAPES(X, ...) X(__bf16, 64, __VA_ARGS__) X(__bf16, 128, __VA_ARGS__) X(_Float16, 64, __VA_ARGS__) X(_Float16, 128, __VA_ARGS__)
template <int FORM_>
struct Form {
  static constexpr int FORM = FORM_;
};
// The one run-time -> compile-time switch of the form: calls f(Form<mask>{}).  No window: the plain varlen form (the only caller without one); else the local
// form or, with slopes, its ALiBi form or, capped (slopes or not), its softcap form — fixed-length or varlen — or, biased (fixed-length only), its dense-bias form.
template <typename F>
static inline auto by_form(bool varlen, bool local, bool alibi, bool capped, bool biased, F&& f) {
  const int form = !local ? FORM_VARLEN : biased ? FORM_LOCAL | FORM_BIAS : FORM_LOCAL | (varlen ? FORM_VARLEN : 0) | (capped ? FORM_SOFTCAP : alibi ? FORM_ALIBI : 0);
#define TFA_BY_FORM(mask) \
  if (form == (mask)) return f(Form<(mask)>{});
  TFA_FORMS_BWD(TFA_BY_FORM)
#undef TFA_BY_FORM
  return f(Form<FORM_VARLEN>{});   // (never: the line above names every value `form` takes)
}

// Local (sliding-window) attention, FlashAttention-2's window: key j is visible to row i iff i + shift - left <= j <= i + shift + right, -1 = unbounded on
// that side, causal forces right = 0.  A side that reaches past every key of every row is unbounded: left >= nk - 1, right >= nq - 1 (max_seqlen for
// varlen).  What is left is FULL (-1, -1), CAUSAL (-1, 0) — the fixed-length and varlen kernels, same bits — or a true window, the LOCAL instantiations.
// Returns the form, or TFA_ERR_SHAPE for a side below -1.
enum { WIN_FULL = 0, WIN_CAUSAL = 1, WIN_LOCAL = 2 };
static inline int window_form(int* left, int* right, bool causal, int nq, int nk) {
  if (*left < -1 || *right < -1) return TFA_ERR_SHAPE;
  if (causal) *right = 0;
  if (*left >= (int64_t)nk - 1) *left = -1;                 // (64 bit: the caller may not have checked nq / nk yet)
  if (*left < 0 && *right == 0) return WIN_CAUSAL;
  if (*right >= (int64_t)nq - 1) *right = -1;
  return (*left < 0 && *right < 0) ? WIN_FULL : WIN_LOCAL;
}
// the window as the kernels read it (KArgs / BArgs::win_left, win_right): both sides >= 0, an unbounded one as nq + nk
template <typename Args>
static inline void set_window(Args* a, int left, int right, int nq, int nk) {
  a->win_left = left < 0 ? nq + nk : left;
  a->win_right = right < 0 ? nq + nk : right;
}

// ALiBi (tfa_fwd_alibi / tfa_bwd_alibi and their varlen forms): one fp32 slope per (batch / sequence, query head) in DEVICE memory, row stride 0 (one row shared
// by the batch) or H.  Checked without reading it: the kernels' work items load their slope themselves (no copy, no synchronisation, graph-capturable).
struct AlibiArg {
  const float* slopes;
  int64_t batch_stride;
  // soft-capping (tfa_fwd_softcap / tfa_bwd_softcap and their varlen forms) rides on the same argument: capped = the call came through a _softcap entry point, which
  // wants softcap > 0 and finite and takes slopes == nullptr as "no bias".  A host scalar, folded into the raw-score domain here (softcap_cr = softcap / scale)
  bool capped = false;
  float softcap = 0.f;
  // the dense bias (tfa_fwd_bias / tfa_bwd_bias) rides on it too: bias != nullptr = the call came through a _bias entry point (no slopes, no cap then)
  const tfa_attn_bias* bias = nullptr;
  bool biased = false;
};
// The dense bias of tfa_fwd_bias / tfa_bwd_bias, checked without reading it: a (b, h) slice is rows of Nk elements at stride[2], through ONE buffer descriptor of
// ((Nq - 1) * stride[2] + Nk) * esize bytes — below 2 GiB — and 8- / 16-byte loads: the base 16-byte aligned, every non-zero stride a multiple of 8 elements.
static inline int check_bias(const tfa_attn_bias* bi, int q_dtype, int Nq, int Nk) {
  if (!bi || !bi->bias) return TFA_ERR_NULL;
  if (bi->dtype != TFA_F32 && bi->dtype != q_dtype) return TFA_ERR_DTYPE;
  if (bi->reserved_ != 0) return TFA_ERR_SHAPE;
  if ((uintptr_t)bi->bias & 15) return TFA_ERR_ALIGN;
  for (int i = 0; i < 3; ++i)
    if (bi->stride[i] < 0 || (bi->stride[i] % 8) != 0) return TFA_ERR_STRIDE;
  if (bi->stride[2] != 0 && bi->stride[2] < Nk) return TFA_ERR_STRIDE;              // (rows that overlap)
  const int esize = bi->dtype == TFA_F32 ? 4 : 2;
  if (bi->stride[2] > (int64_t)0x7fffffff / esize) return TFA_ERR_STRIDE;
  if (((int64_t)Nq - 1) * bi->stride[2] + Nk >= ((int64_t)1 << 31) / esize) return TFA_ERR_STRIDE;   // (64 bit throughout: the caller may not have checked Nq yet)
  return TFA_OK;
}
// ... and into the kernel arguments (KArgs / BArgs: bytes no bias launch reads — after everything else has been written)
template <typename Args>
static inline void set_bias(Args* a, const tfa_attn_bias& bi, int Nq, int Nk) {
  const int esize = bi.dtype == TFA_F32 ? 4 : 2;
  a->bias = bi.bias;
  a->bias_sb = bi.stride[0];
  a->bias_sh = bi.stride[1];
  a->bias_sn = (int)bi.stride[2] * esize;                                           // (bytes)
  a->bias_bytes = (unsigned)((((int64_t)Nq - 1) * bi.stride[2] + Nk) * esize);
  a->bias_f32 = bi.dtype == TFA_F32;
}
static inline int check_alibi(const AlibiArg& al, int H, float scale) {
  if (al.capped) {
    const float cr = al.softcap / scale;
    if (!(al.softcap > 0.f) || !(al.softcap <= 3.0e38f) || !(cr > 0.f) || !(cr <= 3.0e38f)) return TFA_ERR_SCALE;   // (0, negative, NaN, inf; or the cap leaves fp32 over the scale)
    if (!al.slopes) return TFA_OK;
  }
  if (!al.slopes) return TFA_ERR_NULL;
  if ((uintptr_t)al.slopes & 3) return TFA_ERR_ALIGN;
  if (al.batch_stride != 0 && al.batch_stride != H) return TFA_ERR_STRIDE;
  return TFA_OK;
}
template <typename Args>
static inline void set_alibi(Args* a, const AlibiArg& al) {
  a->slopes = al.slopes;
  a->slopes_bs = al.slopes ? (int)al.batch_stride : 0;
  if (al.capped) a->softcap_cr = al.softcap / a->scale;
}

}  // namespace tfa
