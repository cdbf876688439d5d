// tfa_bwd_api.hip — extern "C" backward entry points of include/tfa.h: validate, fill kernel arguments, launch on the caller's stream
//   delta -> dQ (tfa_bwd_kernel.h) -> fused dK/dV (tfa_bwd_kv_kernel.h)                       the default: 7 GEMM units
//   delta -> fused dK/dV that also stores dS -> dQ = dS.K (tfa_bwd_dq_kernel.h)               with tfa_bwd_params::workspace: 5 units
//   delta -> dQ -> dK -> dV (tfa_bwd_kernel.h, three single-gradient launches)                head dims above 128, and the debug form
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "tfa.h"
#include "tfa_bwd_launch.h"

namespace tfa {
template <> hipError_t launch_bwd<__bf16, 64>(const BArgs&, int, int, bool, bool, hipStream_t, bool);
template <> hipError_t launch_bwd<__bf16, 128>(const BArgs&, int, int, bool, bool, hipStream_t, bool);
template <> hipError_t launch_bwd<_Float16, 64>(const BArgs&, int, int, bool, bool, hipStream_t, bool);
template <> hipError_t launch_bwd<_Float16, 128>(const BArgs&, int, int, bool, bool, hipStream_t, bool);
template <> hipError_t launch_bwd<__bf16, 256>(const BArgs&, int, int, bool, bool, hipStream_t, bool);
template <> hipError_t launch_bwd<_Float16, 256>(const BArgs&, int, int, bool, bool, hipStream_t, bool);
template <> hipError_t launch_bwd_kv<__bf16, 64>(const BArgs&, int, bool, bool, hipStream_t, bool);
template <> hipError_t launch_bwd_kv<__bf16, 128>(const BArgs&, int, bool, bool, hipStream_t, bool);
template <> hipError_t launch_bwd_kv<_Float16, 64>(const BArgs&, int, bool, bool, hipStream_t, bool);
template <> hipError_t launch_bwd_kv<_Float16, 128>(const BArgs&, int, bool, bool, hipStream_t, bool);
template <> hipError_t launch_bwd_dq_ws<__bf16, 64>(const BArgs&, int, bool, bool, hipStream_t, bool);
template <> hipError_t launch_bwd_dq_ws<__bf16, 128>(const BArgs&, int, bool, bool, hipStream_t, bool);
template <> hipError_t launch_bwd_dq_ws<_Float16, 64>(const BArgs&, int, bool, bool, hipStream_t, bool);
template <> hipError_t launch_bwd_dq_ws<_Float16, 128>(const BArgs&, int, bool, bool, hipStream_t, bool);
template <> hipError_t launch_delta<__bf16, 64>(const void*, const void*, float*, const long long*, const long long*, int, int, long long, int, hipStream_t, bool);
template <> hipError_t launch_delta<__bf16, 128>(const void*, const void*, float*, const long long*, const long long*, int, int, long long, int, hipStream_t, bool);
template <> hipError_t launch_delta<_Float16, 64>(const void*, const void*, float*, const long long*, const long long*, int, int, long long, int, hipStream_t, bool);
template <> hipError_t launch_delta<_Float16, 128>(const void*, const void*, float*, const long long*, const long long*, int, int, long long, int, hipStream_t, bool);
template <> hipError_t launch_delta<__bf16, 256>(const void*, const void*, float*, const long long*, const long long*, int, int, long long, int, hipStream_t, bool);
template <> hipError_t launch_delta<_Float16, 256>(const void*, const void*, float*, const long long*, const long long*, int, int, long long, int, hipStream_t, bool);
}  // namespace tfa

namespace {

thread_local int g_bwd_split = 0;   // tfa_debug_bwd_split: bit 3 = delta by a launch of its own (not fused into the dQ launch), bit 0 = dK and dV as two launches (the round-1/2 form), bit 1 = force the windowed
                                    // (>= 2 GiB slices) instantiations on any problem; for A/B and parity cross-checks

// extent of one (b,h) slice.  Kernels with one descriptor per slice need every byte offset they form (up to 512 rows past the end)
// inside int32; the BIG instantiations (windowed descriptors, tfa_bwd_kernel.h) only need a window — 768 rows — to fit, and are
// launched when *big comes back set.  big == nullptr: the caller has no windowed form.
bool slice_bytes(int64_t n, int64_t row_stride, int d, int esize, unsigned* out, unsigned long long* full = nullptr, int* big = nullptr) {
  const int64_t bytes = tfa::span_bytes(n - 1, row_stride, d, esize);      // (INT64_MAX when a product leaves 64 bit: refused by size below)
  const int64_t reach = tfa::span_bytes(n + 512, row_stride, d, esize);    // every byte offset a kernel forms stays inside int32
  const int64_t window = tfa::span_bytes(768, row_stride, d, esize);
  if (bytes <= 0) return false;
  if (reach >= (int64_t)0x7fffffff) {
    if (!big || window >= (int64_t)0x7fffffff) return false;
    *big = 1;
  }
  *out = (unsigned)(bytes < (int64_t)0x7fffffff ? bytes : (int64_t)0x7fffffff);
  if (full) *full = (unsigned long long)bytes;
  return true;
}

bool fill(tfa::BTensor* t, const void* ptr, const int64_t* st, int64_t n, int d, int esize, int* big) {
  t->p = ptr;
  t->s_b = st[0]; t->s_h = st[1]; t->s_n = st[2];
  return slice_bytes(n, st[2], d, esize, &t->bytes, &t->full, big);
}

int check_strides(const int64_t* st, int d, int esize) {
  for (int i = 0; i < 3; ++i) {
    if (st[i] < 0) return TFA_ERR_STRIDE;
    if (st[i] % (16 / esize) != 0) return TFA_ERR_STRIDE;
  }
  if (st[2] < d) return TFA_ERR_STRIDE;
  return TFA_OK;
}

// The preconditions every backward form shares, in tfa_bwd's order (an input with several faults gets the status of the first).  v is the problem as the
// kernels see it — varlen: ONE sequence of max_seqlen_q x max_seqlen_k rows, batch stride 0 (run_bwd_varlen).  What differs between the forms:
//   form_ptrs:  the form's own pointers are set (varlen: cu_seqlens);
//   form_shape: the form's own shape conditions hold (a fixed-length window: Nq + Nk < 2^28; varlen: totals > 0, flags and reserved_ 0);
//   max_d:      the widest head dim (256 tfa_bwd, 128 the varlen and local forms);
//   window_st:  the varlen window's status (window_form and its 2^28 limit), reported behind the scale;
//   stat_align: bytes of alignment of lse and delta (16 fixed-length: read as 16-byte vectors; 4 varlen);
//   rows:       rows of lse and delta (B*H*Nq, varlen H*total_q).
int check_bwd(const tfa_bwd_params& v, bool form_ptrs, bool form_shape, int max_d, int window_st, int stat_align, int64_t rows) {
  if (!v.q || !v.k || !v.v || !v.out || !v.dout || !v.lse || !v.dq || !v.dk || !v.dv || !v.delta || !form_ptrs) return TFA_ERR_NULL;
  if (v.dtype != TFA_F16 && v.dtype != TFA_BF16) return TFA_ERR_DTYPE;
  if (v.grad_dtype != v.dtype && v.grad_dtype != TFA_F32) return TFA_ERR_DTYPE;
  if (v.D < 8 || v.D > max_d || (v.D % 8) != 0) return TFA_ERR_HEAD_DIM;   // kernels are 64, 128 and 256 wide; BArgs::dv = the valid part
  if (v.B <= 0 || v.H <= 0 || v.Hk <= 0 || v.Nq <= 0 || v.Nk <= 0 || v.H % v.Hk != 0 || !form_shape) return TFA_ERR_SHAPE;
  if (!(v.softmax_scale > 0.f) || !isfinite(v.softmax_scale)) return TFA_ERR_SCALE;
  if (window_st != TFA_OK) return window_st;
  const int gsz = (v.grad_dtype == TFA_F32) ? 4 : 2;
  const int64_t* st[8] = {v.q_stride, v.k_stride, v.v_stride, v.o_stride, v.do_stride, v.dq_stride, v.dk_stride, v.dv_stride};
  for (int i = 0; i < 8; ++i) {
    const int c = check_strides(st[i], v.D, i < 5 ? 2 : gsz);
    if (c) return c;
  }
  const uintptr_t al = (uintptr_t)v.q | (uintptr_t)v.k | (uintptr_t)v.v | (uintptr_t)v.out | (uintptr_t)v.dout | (uintptr_t)v.dq |
                       (uintptr_t)v.dk | (uintptr_t)v.dv;
  if (al & 15) return TFA_ERR_ALIGN;
  if (((uintptr_t)v.lse | (uintptr_t)v.delta) & (stat_align - 1)) return TFA_ERR_ALIGN;
  if (rows >= (int64_t)0x1fffffff) return TFA_ERR_SHAPE;
  return TFA_OK;
}

// The kernel arguments every launch of v shares — everything but the gradients — after the gradients' slices pass the same size rule as the inputs.
// bigp: slice_bytes's (nullptr: the form has no windowed instantiation).
int fill_args(const tfa_bwd_params& v, int* bigp, tfa::BArgs* a) {
  memset(a, 0, sizeof(*a));
  const int esz = 2, gsz = (v.grad_dtype == TFA_F32) ? 4 : 2;
  // (out: read by the dQ launch when it forms delta and by the delta kernel; fill() is also what validates its strides and slice size for every form)
  if (!fill(&a->q, v.q, v.q_stride, v.Nq, v.D, esz, bigp) || !fill(&a->k, v.k, v.k_stride, v.Nk, v.D, esz, bigp) ||
      !fill(&a->v, v.v, v.v_stride, v.Nk, v.D, esz, bigp) || !fill(&a->out, v.out, v.o_stride, v.Nq, v.D, esz, bigp) ||
      !fill(&a->dout, v.dout, v.do_stride, v.Nq, v.D, esz, bigp))
    return TFA_ERR_STRIDE;
  unsigned tmp;
  unsigned long long tmpf;
  if (!slice_bytes(v.Nq, v.dq_stride[2], v.D, gsz, &tmp, &tmpf, bigp) || !slice_bytes(v.Nk, v.dk_stride[2], v.D, gsz, &tmp, &tmpf, bigp) ||
      !slice_bytes(v.Nk, v.dv_stride[2], v.D, gsz, &tmp, &tmpf, bigp))
    return TFA_ERR_STRIDE;
  a->lse = v.lse; a->delta = v.delta; a->delta_w = v.delta;
  a->B = v.B; a->H = v.H; a->Hk = v.Hk; a->Nq = v.Nq; a->Nk = v.Nk;
  a->dv = v.D;
  a->scale = v.softmax_scale;
  a->scale_log2 = v.softmax_scale * 1.4426950408889634f;
  return TFA_OK;
}

// bytes of the dS workspace for *p, 0 when a head's slab (roundup(Nk,128) x roundup(Nq,256) x 2 bytes) would not fit one descriptor
long long ws_bytes(const tfa_bwd_params* p, int* nk_pad, int* nq_pad) {
  const long long nk = ((long long)p->Nk + 127) / 128 * 128, nq = ((long long)p->Nq + 255) / 256 * 256;
  if (nk_pad) *nk_pad = (int)nk;
  if (nq_pad) *nq_pad = (int)nq;
  if (nk * nq * 2 >= (long long)0x7fffffff) return 0;
  return tfa::size_product({p->B, p->H, nk, nq, 2});
}

// ws_need (optional): receives the bytes of dS scratch the 5-GEMM form would use for *p, 0 when this problem never takes that form
int run_bwd(const tfa_bwd_params* p, void* stream, bool dry, long long* ws_need = nullptr) {
  if (ws_need) *ws_need = 0;
  if (!p) return TFA_ERR_NULL;
  int st = check_bwd(*p, true, true, 256, TFA_OK, 16, tfa::sat_mul((int64_t)p->B * p->H, p->Nq));
  if (st) return st;
  const int gsz = (p->grad_dtype == TFA_F32) ? 4 : 2;
  tfa::BArgs a;
  // slices of 2 GiB and more (long (B,N,H,D) tensors): the windowed instantiations of the dQ launch and of the fused dK/dV launch —
  // not with the two-launch debug form at head dims up to 128 (its dK / dV launches have no windowed instantiation; the 256-wide kernel has one for each of its three launches)
  const bool can_big = p->D > 128 || !(g_bwd_split & 1);
  int big = (g_bwd_split & 2) ? 1 : 0;        // tests: the windowed instantiations on a small problem
  int* bigp = can_big ? &big : nullptr;
  st = fill_args(*p, bigp, &a);
  if (st) return st;
  if (big && !can_big) return TFA_ERR_STRIDE;
  a.big = big;
  const bool wide256 = p->D > 128;          // head dims 136..256: one wave per SIMD, 128-row resident blocks, three single-gradient launches
  const bool causal = p->is_causal != 0, f32 = p->grad_dtype == TFA_F32;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);

  auto launch = [&](int mode, void* grad, const int64_t* gst, int n_res, int h_res) -> int {
    tfa::BArgs m = a;
    m.grad = grad; m.gs_b = gst[0]; m.gs_h = gst[1]; m.gs_n = gst[2];
    if (!slice_bytes(n_res, gst[2], p->D, gsz, &m.g_bytes, &m.g_full, bigp)) return TFA_ERR_STRIDE;
    const int res_rows = wide256 ? 128 : 256;
    m.nrb = (n_res + res_rows - 1) / res_rows;
    const int64_t grid = (int64_t)p->B * h_res * m.nrb;
    if (grid >= (int64_t)0x7fffffff) return TFA_ERR_SHAPE;
    return (int)tfa::by_dtype_width<64, 128, 256>(p->dtype, p->D, [&](auto k) {
      return tfa::launch_bwd<typename decltype(k)::T, decltype(k)::W>(m, mode, (int)grid, causal, f32, s, dry);
    });
  };

  // the fused dK/dV launch (head dims up to 128; a.ws: the form that also writes dS)
  auto launch_kv = [&](const tfa::BArgs& m, int grid) {
    return tfa::by_dtype_width<64, 128>(p->dtype, p->D, [&](auto k) {
      return tfa::launch_bwd_kv<typename decltype(k)::T, decltype(k)::W>(m, grid, causal, f32, s, dry);
    });
  };

  // ---- with a workspace: dK/dV launch that also writes dS, then dQ = scale * dS . K (5 GEMM units) -----------------------------
  int nk_pad = 0, nq_pad = 0;
  const long long need = ws_bytes(p, &nk_pad, &nq_pad);
  if (p->workspace && (((uintptr_t)p->workspace) & 15)) return TFA_ERR_ALIGN;
#if defined(TFA_BWD_TRACE)
  // debug build: with bit 2 of tfa_debug_bwd_split the LAST 64 MiB of the workspace receive the fused launch's per-wave wait cycles
  constexpr long long kTraceBytes = 64ll << 20;
  const bool tracing = (g_bwd_split & 4) && p->workspace && p->workspace_bytes >= kTraceBytes;
  const long long ws_avail = p->workspace_bytes - (tracing ? kTraceBytes : 0);
  a.tr = tracing ? reinterpret_cast<char*>(p->workspace) + ws_avail : nullptr;
#else
  const long long ws_avail = p->workspace_bytes;
#endif
  // the kept-dS form exists for head dims up to 128, slices below 2 GiB, and not with the two-launch debug form
  const bool ws_form = need > 0 && !(g_bwd_split & 1) && !wide256 && !big;
  if (ws_need) *ws_need = ws_form ? need : 0;
  const bool use_ws = p->workspace != nullptr && ws_form && ws_avail >= need;
  // delta = rowsum(dout o out): the dQ launch computes it from its resident dO rows and the O rows and writes it for the launches behind it
  // (BArgs::fuse_delta; 51 us and one pass over dO less at config 3) — unless the fused dK/dV launch runs FIRST (the workspace form), or
  // tfa_debug_bwd_split value 8 (bit 3) asks for the launch of its own (A/B, tests)
  const bool fuse_delta = !use_ws && !(g_bwd_split & 8);
  a.fuse_delta = fuse_delta ? 1 : 0;
  if (!fuse_delta)
  {
    const long long os[3] = {p->o_stride[0], p->o_stride[1], p->o_stride[2]};
    const long long ds[3] = {p->do_stride[0], p->do_stride[1], p->do_stride[2]};
    const long long rows = (long long)p->B * p->H * p->Nq;
    const hipError_t e = tfa::by_dtype_width<64, 128, 256>(p->dtype, p->D, [&](auto k) {
      return tfa::launch_delta<typename decltype(k)::T, decltype(k)::W>(p->out, p->dout, p->delta, os, ds, p->H, p->Nq, rows, p->D, s, dry);
    });
    if (e != hipSuccess) return (int)e;
  }
  if (use_ws) {
    tfa::BArgs m = a;
    m.ws = p->workspace; m.ws_nk = nk_pad; m.ws_nq = nq_pad;
    m.grad = p->dk; m.gs_b = p->dk_stride[0]; m.gs_h = p->dk_stride[1]; m.gs_n = p->dk_stride[2];
    m.grad2 = p->dv; m.g2s_b = p->dv_stride[0]; m.g2s_h = p->dv_stride[1]; m.g2s_n = p->dv_stride[2];
    if (!slice_bytes(p->Nk, p->dk_stride[2], p->D, gsz, &m.g_bytes) || !slice_bytes(p->Nk, p->dv_stride[2], p->D, gsz, &m.g2_bytes)) return TFA_ERR_STRIDE;
    m.nrb = (p->Nk + 127) / 128;
    int64_t grid = (int64_t)p->B * p->Hk * m.nrb;
    if (grid >= (int64_t)0x7fffffff) return TFA_ERR_SHAPE;
    hipError_t e = launch_kv(m, (int)grid);
    if (e != hipSuccess) return (int)e;
    tfa::BArgs d = a;
    d.ws = p->workspace; d.ws_nk = nk_pad; d.ws_nq = nq_pad;
    d.grad = p->dq; d.gs_b = p->dq_stride[0]; d.gs_h = p->dq_stride[1]; d.gs_n = p->dq_stride[2];
    if (!slice_bytes(p->Nq, p->dq_stride[2], p->D, gsz, &d.g_bytes)) return TFA_ERR_STRIDE;
    d.nrb = (p->Nq + 255) / 256;
    grid = (int64_t)p->B * p->H * d.nrb;
    if (grid >= (int64_t)0x7fffffff) return TFA_ERR_SHAPE;
    e = tfa::by_dtype_width<64, 128>(p->dtype, p->D, [&](auto k) {
      return tfa::launch_bwd_dq_ws<typename decltype(k)::T, decltype(k)::W>(d, (int)grid, causal, f32, s, dry);
    });
    return (int)e;
  }
  st = launch(tfa::BWD_DQ, p->dq, p->dq_stride, p->Nq, p->H);
  if (st) return st;
  if ((g_bwd_split & 1) || wide256) {                            // head dims above 128, and debug / A-B: the two single-gradient launches (S computed twice)
    st = launch(tfa::BWD_DK, p->dk, p->dk_stride, p->Nk, p->Hk);
    if (st) return st;
    return launch(tfa::BWD_DV, p->dv, p->dv_stride, p->Nk, p->Hk);
  }
  // dK and dV in one launch: S and dP once each (tfa_bwd_kv_kernel.h)
  tfa::BArgs m = a;
  m.grad = p->dk; m.gs_b = p->dk_stride[0]; m.gs_h = p->dk_stride[1]; m.gs_n = p->dk_stride[2];
  m.grad2 = p->dv; m.g2s_b = p->dv_stride[0]; m.g2s_h = p->dv_stride[1]; m.g2s_n = p->dv_stride[2];
  if (!slice_bytes(p->Nk, p->dk_stride[2], p->D, gsz, &m.g_bytes, &m.g_full, bigp) ||
      !slice_bytes(p->Nk, p->dv_stride[2], p->D, gsz, &m.g2_bytes, &m.g2_full, bigp)) return TFA_ERR_STRIDE;
  constexpr int kv_keys = 32 * TFA_BWD_KV_KG_OF(false);   // resident keys per workgroup of the fused launch
  m.nrb = (int)(((int64_t)p->Nk + kv_keys - 1) / kv_keys);
  const int64_t grid = (int64_t)p->B * p->Hk * m.nrb;
  if (grid >= (int64_t)0x7fffffff) return TFA_ERR_SHAPE;
  return (int)launch_kv(m, (int)grid);
}

// The varlen and local forms: the dQ launch (which forms delta) and then the fused dK/dV launch of the form kernels (VARLEN / LOCAL instantiations:
// tfa_bwd_form_inst.inc).  a holds everything but the gradients; v is the problem as the kernels see it (run_bwd_varlen: one sequence, batch stride 0).
// alibi: the ALiBi form of the local kernels (a.slopes set; local is then true whatever the window); capped: their soft-capping form instead (a.softcap_cr set,
// a.slopes set or null)
int launch_form_pair(const tfa::BArgs& a, const tfa_bwd_params& v, bool varlen, bool local, bool alibi, bool capped, void* stream, bool dry, bool biased = false) {
  const int gsz = (v.grad_dtype == TFA_F32) ? 4 : 2;
  const bool causal = v.is_causal != 0, f32 = v.grad_dtype == TFA_F32;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  auto run = [&](const tfa::BArgs& m, bool keys, int64_t grid) -> int {
    if (grid >= (int64_t)0x7fffffff) return TFA_ERR_SHAPE;
    return (int)tfa::by_dtype_width<64, 128>(v.dtype, v.D, [&](auto k) {
      using T = typename decltype(k)::T;
      constexpr int W = decltype(k)::W;
      return tfa::by_form(varlen, local, alibi, capped, biased, [&](auto form) {
        return tfa::launch_bwd_form<T, W, decltype(form)::FORM>(m, keys, (int)grid, causal, f32, s, dry);
      });
    });
  };
  // dQ (and delta): 256-row resident blocks of each (sequence, query head)
  tfa::BArgs d = a;
  d.grad = v.dq; d.gs_b = v.dq_stride[0]; d.gs_h = v.dq_stride[1]; d.gs_n = v.dq_stride[2];
  if (!slice_bytes(v.Nq, d.gs_n, v.D, gsz, &d.g_bytes)) return TFA_ERR_STRIDE;   // (no g_full: varlen keeps cu_q / cu_k in its bytes)
  d.nrb = (v.Nq + 255) / 256;
  // dK and dV in one launch: 32 * KG resident keys of each (sequence, K/V head)
  tfa::BArgs m = a;
  m.grad = v.dk; m.gs_b = v.dk_stride[0]; m.gs_h = v.dk_stride[1]; m.gs_n = v.dk_stride[2];
  m.grad2 = v.dv; m.g2s_b = v.dv_stride[0]; m.g2s_h = v.dv_stride[1]; m.g2s_n = v.dv_stride[2];
  if (!slice_bytes(v.Nk, m.gs_n, v.D, gsz, &m.g_bytes) || !slice_bytes(v.Nk, m.g2s_n, v.D, gsz, &m.g2_bytes)) return TFA_ERR_STRIDE;
  constexpr int kv_keys = 32 * TFA_BWD_KV_KG_OF(false);
  m.nrb = (v.Nk + kv_keys - 1) / kv_keys;
  const int st_dq = run(d, false, (int64_t)v.B * v.H * d.nrb);
  if (st_dq) return st_dq;
  return run(m, true, (int64_t)v.B * v.Hk * m.nrb);
}

// Local (sliding-window) attention, tfa_bwd_local: the window's form as the forward sees it (tfa_host_util.h: window_form) — FULL / CAUSAL run tfa_bwd's own
// launches, a true window the LOCAL instantiations (every slice within one descriptor: no windowed local form)
// tfa_bwd_alibi (al): every window, FULL and CAUSAL included, runs the ALiBi form of the local kernels
int run_bwd_local(const tfa_bwd_params* p, const int* w, const tfa::AlibiArg* al, void* stream, bool dry) {
  if (!p) return TFA_ERR_NULL;
  int win[2] = {w[0], w[1]};
  const int form = tfa::window_form(&win[0], &win[1], p->is_causal != 0, p->Nq, p->Nk);
  if (form < 0) return form;
  if (form != tfa::WIN_LOCAL && !al) {
    tfa_bwd_params f = *p;
    f.is_causal = form == tfa::WIN_CAUSAL;
    return run_bwd(&f, stream, dry);
  }
  int st = check_bwd(*p, true, (int64_t)p->Nq + p->Nk < (1 << 28), 128, TFA_OK, 16, tfa::sat_mul((int64_t)p->B * p->H, p->Nq));
  if (st) return st;
  if (al && (st = al->biased ? tfa::check_bias(al->bias, p->dtype, p->Nq, p->Nk) : tfa::check_alibi(*al, p->H, p->softmax_scale)) != TFA_OK) return st;
  tfa::BArgs a;
  st = fill_args(*p, nullptr, &a);
  if (st) return st;
  a.fuse_delta = 1;                                  // (the dQ launch forms delta)
  tfa::set_window(&a, win[0], win[1], p->Nq, p->Nk);
  if (al && al->biased) tfa::set_bias(&a, *al->bias, p->Nq, p->Nk);   // (tfa_bwd_bias: in bytes no local launch reads, the slopes' among them)
  else if (al) tfa::set_alibi(&a, *al);
  return launch_form_pair(a, *p, false, true, al != nullptr, al && al->capped, stream, dry, al && al->biased);
}

// Packed variable-length batches (include/tfa.h: tfa_bwd_varlen, tfa_bwd_varlen_local — w: the window, or nullptr): as in the forward (tfa_api.hip: run_varlen)
// the host checks ONE sequence of max_seqlen_q x max_seqlen_k rows — every slice must fit one descriptor, there is no windowed varlen form — sizes the grids
// from it and never reads cu_seqlens: each work item reads its sequence's bounds itself.
int run_bwd_varlen(const tfa_varlen_bwd_params* p, const int* w, const tfa::AlibiArg* al, void* stream, bool dry) {
  if (!p) return TFA_ERR_NULL;
  tfa_bwd_params v;                                  // the fixed-length view: (head, row) strides as (batch, head, row) triples, batch stride 0
  memset(&v, 0, sizeof(v));
  v.q = p->q; v.k = p->k; v.v = p->v; v.out = p->out; v.dout = p->dout; v.lse = p->lse; v.dq = p->dq; v.dk = p->dk; v.dv = p->dv; v.delta = p->delta;
  v.B = p->B; v.H = p->H; v.Hk = p->Hk; v.Nq = p->max_seqlen_q; v.Nk = p->max_seqlen_k; v.D = p->D;
  const int64_t* src[8] = {p->q_stride, p->k_stride, p->v_stride, p->o_stride, p->do_stride, p->dq_stride, p->dk_stride, p->dv_stride};
  int64_t* dst[8] = {v.q_stride, v.k_stride, v.v_stride, v.o_stride, v.do_stride, v.dq_stride, v.dk_stride, v.dv_stride};
  for (int i = 0; i < 8; ++i) { dst[i][0] = 0; dst[i][1] = src[i][0]; dst[i][2] = src[i][1]; }
  v.softmax_scale = p->softmax_scale; v.dtype = p->dtype; v.grad_dtype = p->grad_dtype;
  int win[2] = {-1, -1}, form = p->is_causal ? tfa::WIN_CAUSAL : tfa::WIN_FULL, window_st = TFA_OK;
  if (w) {
    win[0] = w[0];
    win[1] = w[1];
    form = tfa::window_form(&win[0], &win[1], p->is_causal != 0, p->max_seqlen_q, p->max_seqlen_k);
    window_st = form < 0 ? form : ((form == tfa::WIN_LOCAL || al) && (int64_t)p->max_seqlen_q + p->max_seqlen_k >= (1 << 28)) ? TFA_ERR_SHAPE : TFA_OK;
  }
  const bool local = form == tfa::WIN_LOCAL || al;   // (the ALiBi kernels are a form of the local ones, whatever the window)
  v.is_causal = form == tfa::WIN_CAUSAL;
  const bool shape = p->total_q > 0 && p->total_k > 0 && p->flags == 0 && p->reserved_ == 0;
  int st = check_bwd(v, p->cu_seqlens_q && p->cu_seqlens_k, shape, 128, window_st, 4, (int64_t)p->H * p->total_q);
  if (st) return st;
  if (al && (st = tfa::check_alibi(*al, p->H, p->softmax_scale)) != TFA_OK) return st;
  tfa::BArgs a;
  st = fill_args(v, nullptr, &a);
  if (st) return st;
  a.fuse_delta = 1;                                  // (the dQ launch forms delta; no separate delta launch in varlen form)
  a.cu_q = p->cu_seqlens_q; a.cu_k = p->cu_seqlens_k;
  a.total_q = p->total_q; a.total_k = p->total_k;   // (BArgs: in the bytes of the windowed / workspace forms' fields, which varlen launches never read)
  if (local) tfa::set_window(&a, win[0], win[1], v.Nq, v.Nk);
  if (al) tfa::set_alibi(&a, *al);
  return launch_form_pair(a, v, true, local, al != nullptr, al && al->capped, stream, dry);
}

}  // namespace

extern "C" {

int tfa_bwd(const tfa_bwd_params* p, void* stream) { return run_bwd(p, stream, false); }
int tfa_bwd_plan(const tfa_bwd_params* p) { return run_bwd(p, nullptr, true); }
int tfa_bwd_varlen(const tfa_varlen_bwd_params* p, void* stream) { return run_bwd_varlen(p, nullptr, nullptr, stream, false); }
int tfa_bwd_local(const tfa_bwd_params* p, int window_left, int window_right, void* stream) {
  const int w[2] = {window_left, window_right};
  return run_bwd_local(p, w, nullptr, stream, false);
}
int tfa_bwd_local_plan(const tfa_bwd_params* p, int window_left, int window_right) {
  const int w[2] = {window_left, window_right};
  return run_bwd_local(p, w, nullptr, nullptr, true);
}
int tfa_bwd_varlen_local(const tfa_varlen_bwd_params* p, int window_left, int window_right, void* stream) {
  const int w[2] = {window_left, window_right};
  return run_bwd_varlen(p, w, nullptr, stream, false);
}
int tfa_bwd_varlen_local_plan(const tfa_varlen_bwd_params* p, int window_left, int window_right) {
  const int w[2] = {window_left, window_right};
  return run_bwd_varlen(p, w, nullptr, nullptr, true);
}
int tfa_bwd_bias(const tfa_bwd_params* p, const tfa_attn_bias* bias, int window_left, int window_right, void* stream) {
  const int w[2] = {window_left, window_right};
  tfa::AlibiArg al{};
  al.bias = bias; al.biased = true;
  return run_bwd_local(p, w, &al, stream, false);
}
int tfa_bwd_bias_plan(const tfa_bwd_params* p, const tfa_attn_bias* bias, int window_left, int window_right) {
  const int w[2] = {window_left, window_right};
  tfa::AlibiArg al{};
  al.bias = bias; al.biased = true;
  return run_bwd_local(p, w, &al, nullptr, true);
}
int tfa_bwd_alibi(const tfa_bwd_params* p, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right, void* stream) {
  const int w[2] = {window_left, window_right};
  const tfa::AlibiArg al{alibi_slopes, slopes_batch_stride};
  return run_bwd_local(p, w, &al, stream, false);
}
int tfa_bwd_alibi_plan(const tfa_bwd_params* p, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right) {
  const int w[2] = {window_left, window_right};
  const tfa::AlibiArg al{alibi_slopes, slopes_batch_stride};
  return run_bwd_local(p, w, &al, nullptr, true);
}
int tfa_bwd_varlen_alibi(const tfa_varlen_bwd_params* p, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right, void* stream) {
  const int w[2] = {window_left, window_right};
  const tfa::AlibiArg al{alibi_slopes, slopes_batch_stride};
  return run_bwd_varlen(p, w, &al, stream, false);
}
int tfa_bwd_varlen_alibi_plan(const tfa_varlen_bwd_params* p, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right) {
  const int w[2] = {window_left, window_right};
  const tfa::AlibiArg al{alibi_slopes, slopes_batch_stride};
  return run_bwd_varlen(p, w, &al, nullptr, true);
}
int tfa_bwd_softcap(const tfa_bwd_params* p, float softcap, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right,
                    void* stream) {
  const int w[2] = {window_left, window_right};
  const tfa::AlibiArg al{alibi_slopes, slopes_batch_stride, true, softcap};
  return run_bwd_local(p, w, &al, stream, false);
}
int tfa_bwd_softcap_plan(const tfa_bwd_params* p, float softcap, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left, int window_right) {
  const int w[2] = {window_left, window_right};
  const tfa::AlibiArg al{alibi_slopes, slopes_batch_stride, true, softcap};
  return run_bwd_local(p, w, &al, nullptr, true);
}
int tfa_bwd_varlen_softcap(const tfa_varlen_bwd_params* p, float softcap, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left,
                           int window_right, void* stream) {
  const int w[2] = {window_left, window_right};
  const tfa::AlibiArg al{alibi_slopes, slopes_batch_stride, true, softcap};
  return run_bwd_varlen(p, w, &al, stream, false);
}
int tfa_bwd_varlen_softcap_plan(const tfa_varlen_bwd_params* p, float softcap, const float* alibi_slopes, int64_t slopes_batch_stride, int window_left,
                                int window_right) {
  const int w[2] = {window_left, window_right};
  const tfa::AlibiArg al{alibi_slopes, slopes_batch_stride, true, softcap};
  return run_bwd_varlen(p, w, &al, nullptr, true);
}
int tfa_debug_bwd_split(int on) { g_bwd_split = on & 15; return TFA_OK; }
long long tfa_bwd_workspace_bytes(const tfa_bwd_params* p) {
  tfa_bwd_params q;
  if (!p) return TFA_ERR_NULL;
  q = *p;
  q.workspace = nullptr;
  long long need = 0;
  const int st = run_bwd(&q, nullptr, true, &need);     // 0 where run_bwd would ignore a workspace (D > 128, slices of 2 GiB and more, debug forms)
  if (st) return st;
  return need;
}

int tfa_bwd_work(const tfa_bwd_params* p, double* flops, double* bytes) {
  const int st = run_bwd(p, nullptr, true);
  if (st) return st;
  const double heads = (double)p->B * p->H, f = p->is_causal ? 0.5 : 1.0;
  if (flops) *flops = 10.0 * heads * p->Nq * (double)p->Nk * p->D * f;
  if (bytes) {
    const double gsz = p->grad_dtype == TFA_F32 ? 4.0 : 2.0;
    const double qrows = heads * p->Nq * p->D, krows = (double)p->B * p->Hk * p->Nk * p->D;
    *bytes = 2.0 * (3.0 * qrows + 2.0 * krows) + gsz * (qrows + 2.0 * krows) + 4.0 * heads * p->Nq;
  }
  return TFA_OK;
}

int tfa_bwd_time(const tfa_bwd_params* p, int warmup, int iters, void* stream, float* avg_ms) {
  if (!avg_ms || iters <= 0 || warmup < 0) return TFA_ERR_NULL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  for (int i = 0; i < warmup; ++i) { const int st = run_bwd(p, stream, false); if (st) return st; }
  hipEvent_t e0, e1;
  hipError_t e = hipEventCreate(&e0);
  if (e != hipSuccess) return (int)e;
  e = hipEventCreate(&e1);
  if (e != hipSuccess) { (void)hipEventDestroy(e0); return (int)e; }
  int st = 0;
  (void)hipEventRecord(e0, s);
  for (int i = 0; i < iters && st == 0; ++i) st = run_bwd(p, stream, false);
  (void)hipEventRecord(e1, s);
  e = hipEventSynchronize(e1);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (st) return st;
  if (e != hipSuccess) return (int)e;
  *avg_ms = ms / (float)iters;
  return TFA_OK;
}

}  // extern "C"
