/*
 * tfa_host.c — a host program for the C ABI of include/tfa.h without Python and without torch: plain C99, tfa.h, the HIP runtime API and libc.
 *
 *   tfa_host run <in> <out>    read one problem, run tfa_fwd_bhnd / tfa_fwd_bhnd_f32out on a stream of its own, write out and lse
 *   tfa_host plan              walk a table of descriptors through every host-only entry point (nothing is allocated on a device, nothing launched)
 *
 * <in>:   12 little-endian 32-bit words {magic "TFAH", dtype (tfa_dtype), B, H, N, D, is_causal, f32out, softmax_scale (float bits), want_lse, 0, 0},
 *         then q, k, v, each B*H*N*D elements of dtype, contiguous (B,H,N,D).
 * <out>:  out — B*H*N*D elements, fp32 when f32out != 0 or dtype == TFA_F32, else of dtype — then, when want_lse, lse: B*H*N floats.
 * Exit 0 on success; a non-zero tfa_* or HIP status is printed to stderr through tfa_strerror and the program exits 1 (usage / file errors: 2).
 *
 * plan: every status is printed (one line per table row: its calls by answer); the program exits 1 if an entry point answers anything that is neither a success (TFA_OK, or a count / variant / rule >= 0
 * from the entry points that return one) nor a negative tfa_status.  It is the program tests/c_host's sanitized build runs (make host-sanitized).
 */
#include <hip/hip_runtime_api.h>
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tfa.h"

#define MAGIC 0x48414654 /* "TFAH" */

/* ---- run ---------------------------------------------------------------------------------------------------------------------------------------- */
static int fail_status(const char* what, int st) {
  fprintf(stderr, "tfa_host: %s: status %d: %s\n", what, st, tfa_strerror(st));
  return 1;
}
#define HIP_DO(call)                                                  \
  do {                                                                \
    hipError_t e_ = (call);                                           \
    if (e_ != hipSuccess) { rc = fail_status(#call, (int)e_); goto done; } \
  } while (0)

static int run_mode(const char* in_path, const char* out_path) {
  int rc = 2;
  int32_t hdr[12];
  void *hq = NULL, *ho = NULL, *dq = NULL, *dk = NULL, *dv = NULL, *dout = NULL;
  float *hl = NULL, *dl = NULL;
  hipStream_t stream = NULL;
  FILE* f = fopen(in_path, "rb");
  if (!f) { perror(in_path); return 2; }
  if (fread(hdr, sizeof(int32_t), 12, f) != 12 || hdr[0] != MAGIC) { fprintf(stderr, "tfa_host: %s: bad header\n", in_path); fclose(f); return 2; }
  const int dtype = hdr[1], B = hdr[2], H = hdr[3], N = hdr[4], D = hdr[5], causal = hdr[6], f32out = hdr[7], want_lse = hdr[9];
  float scale;
  memcpy(&scale, &hdr[8], sizeof(float));
  if (B <= 0 || H <= 0 || N <= 0 || D <= 0 || (int64_t)B * H * N * D > (int64_t)1 << 28 || dtype < TFA_F16 || dtype > TFA_F32) {
    fprintf(stderr, "tfa_host: %s: sizes out of range for this program\n", in_path);
    fclose(f);
    return 2;
  }
  const size_t n = (size_t)B * H * N * D, rows = (size_t)B * H * N;
  const size_t esize = dtype == TFA_F32 ? 4 : 2, osize = (f32out || dtype == TFA_F32) ? 4 : 2;
  hq = malloc(3 * n * esize);
  ho = malloc(n * osize);
  hl = (float*)malloc(rows * sizeof(float));
  if (!hq || !ho || !hl || fread(hq, esize, 3 * n, f) != 3 * n) { fprintf(stderr, "tfa_host: %s: short read\n", in_path); fclose(f); goto done; }
  fclose(f);
  rc = 1;
  HIP_DO(hipStreamCreate(&stream));
  HIP_DO(hipMalloc(&dq, n * esize));
  HIP_DO(hipMalloc(&dk, n * esize));
  HIP_DO(hipMalloc(&dv, n * esize));
  HIP_DO(hipMalloc(&dout, n * osize));
  HIP_DO(hipMalloc((void**)&dl, rows * sizeof(float)));
  HIP_DO(hipMemcpy(dq, hq, n * esize, hipMemcpyHostToDevice));
  HIP_DO(hipMemcpy(dk, (char*)hq + n * esize, n * esize, hipMemcpyHostToDevice));
  HIP_DO(hipMemcpy(dv, (char*)hq + 2 * n * esize, n * esize, hipMemcpyHostToDevice));
  {
    const int rc_call = f32out ? tfa_fwd_bhnd_f32out(dq, dk, dv, (float*)dout, want_lse ? dl : NULL, B, H, N, D, scale, causal, dtype, stream)
                          : tfa_fwd_bhnd(dq, dk, dv, dout, want_lse ? dl : NULL, B, H, N, D, scale, causal, dtype, stream);
    if (rc_call != TFA_OK) { rc = fail_status(f32out ? "tfa_fwd_bhnd_f32out" : "tfa_fwd_bhnd", rc_call); goto done; }
  }
  HIP_DO(hipStreamSynchronize(stream));
  HIP_DO(hipMemcpy(ho, dout, n * osize, hipMemcpyDeviceToHost));
  if (want_lse) HIP_DO(hipMemcpy(hl, dl, rows * sizeof(float), hipMemcpyDeviceToHost));
  f = fopen(out_path, "wb");
  if (!f) { perror(out_path); rc = 2; goto done; }
  if (fwrite(ho, osize, n, f) != n || (want_lse && fwrite(hl, sizeof(float), rows, f) != rows)) { fprintf(stderr, "tfa_host: %s: short write\n", out_path); rc = 2; }
  else rc = 0;
  if (fclose(f) != 0) rc = 2;
done:
  if (dq) (void)hipFree(dq);
  if (dk) (void)hipFree(dk);
  if (dv) (void)hipFree(dv);
  if (dout) (void)hipFree(dout);
  if (dl) (void)hipFree(dl);
  if (stream) (void)hipStreamDestroy(stream);
  free(hq);
  free(ho);
  free(hl);
  return rc;
}

/* ---- plan --------------------------------------------------------------------------------------------------------------------------------------- */
static int g_bad = 0, g_calls = 0;
static char g_row[96] = "";

/* one line per row of the table: how many of its calls succeeded and how many answered each tfa_status; an answer that is neither is printed with its entry
 * point.  Flushed when the row changes, so the last line in front of a sanitizer report names the row before the one that raised it. */
static int g_row_calls = 0, g_row_ok = 0, g_row_status[9];

static void flush_row(void) {
  if (g_row_calls) {
    printf("%-36s %4d calls: %4d ok", g_row, g_row_calls, g_row_ok);
    for (int i = 1; i <= 8; ++i)
      if (g_row_status[i]) printf(", %d x%d", -i, g_row_status[i]);
    printf("\n");
  }
  g_row_calls = g_row_ok = 0;
  memset(g_row_status, 0, sizeof(g_row_status));
  fflush(stdout);
}
static void set_row(const char* kind, const char* name) {
  flush_row();
  snprintf(g_row, sizeof(g_row), "%s %s", kind, name);
}
static void record(const char* fn, long long s, int ok) {
  ++g_row_calls, ++g_calls;
  if (!ok) {
    printf("%-36s %s answered %lld: neither a success nor a tfa_status\n", g_row, fn, s);
    ++g_bad;
  } else if (s >= 0) ++g_row_ok;
  else ++g_row_status[-s];
}
/* an entry point that answers a status: TFA_OK or a negative tfa_status */
static void st(const char* fn, long long s) { record(fn, s, s == TFA_OK || (s <= TFA_ERR_NULL && s >= TFA_ERR_SCALE)); }
/* an entry point that answers a count, a variant or a rule (>= 0), or a negative tfa_status */
static void cnt(const char* fn, long long s) { record(fn, s, s >= 0 || (s <= TFA_ERR_NULL && s >= TFA_ERR_SCALE)); }

static float quiet_nan(void) { return strtof("nan", NULL); }
static void* fake(int i) { return (void*)(uintptr_t)(0x10000000u + 0x100000u * (unsigned)i); } /* never dereferenced: nothing here launches */

static int64_t smul(int64_t a, int64_t b) { /* a * b for non-negative operands, saturating at INT64_MAX / 2 (the table's own arithmetic must not overflow) */
  if (a == 0 || b == 0) return 0;
  return a > (INT64_MAX / 2) / b ? INT64_MAX / 2 : a * b;
}
static void contig(int64_t* s, int64_t H, int64_t N, int64_t D) { s[0] = smul(smul(H, N), D); s[1] = smul(N, D); s[2] = D; }

enum { M_NONE, M_NULL_PARAMS, M_NULL_Q, M_NULL_OUT, M_MISALIGNED, M_ROW_BELOW_D, M_NEG_STRIDE, M_ODD_STRIDE, M_HUGE_STRIDE, M_SCALE_NAN, M_SCALE_ZERO, M_RESERVED,
       M_FLAGS, M_KV_OFFSET, M_OUT_F32, M_BAD_DTYPE, M_NULL_AUX, M_MISALIGNED_AUX, M_BNHD };

typedef struct shape { const char* name; int dtype, B, H, Hk, Nq, Nk, D, causal, mut; } shape;

static const shape SHAPES[] = {
    /* the shapes the ABI tests and the GPU tests use */
    {"headline", TFA_BF16, 4, 32, 32, 4096, 4096, 128, 1, M_NONE},
    {"bhnd-320-d128", TFA_BF16, 2, 4, 4, 320, 320, 128, 1, M_NONE},
    {"bhnd-192-d64", TFA_F16, 1, 2, 2, 192, 192, 64, 0, M_NONE},
    {"bhnd-257-d40", TFA_BF16, 1, 2, 2, 257, 257, 40, 1, M_NONE},
    {"bhnd-200-d256", TFA_F16, 1, 2, 2, 200, 200, 256, 1, M_NONE},
    {"f32-70-d72", TFA_F32, 1, 2, 2, 70, 70, 72, 1, M_NONE},
    {"gqa-320x385", TFA_BF16, 1, 4, 2, 320, 385, 128, 1, M_NONE},
    {"gqa-bnhd", TFA_F16, 2, 8, 2, 257, 130, 96, 0, M_BNHD},
    {"decode-gqa", TFA_BF16, 1, 32, 8, 1, 16384, 128, 0, M_NONE},
    {"chunk-route", TFA_BF16, 1, 8, 4, 3, 6000, 256, 1, M_NONE},
    {"d136", TFA_F16, 1, 2, 1, 70, 203, 136, 1, M_NONE},
    {"one-row-one-key", TFA_F16, 1, 1, 1, 1, 1, 8, 1, M_NONE},
    {"f32-out", TFA_BF16, 1, 2, 2, 192, 192, 128, 0, M_OUT_F32},
    {"exact-max", TFA_BF16, 4, 32, 32, 4096, 4096, 128, 1, M_FLAGS},
    {"kv-offset", TFA_BF16, 1, 2, 2, 70, 203, 64, 1, M_KV_OFFSET},
    /* refusals */
    {"null-params", TFA_BF16, 1, 2, 2, 64, 64, 64, 0, M_NULL_PARAMS},
    {"null-q", TFA_BF16, 1, 2, 2, 64, 64, 64, 0, M_NULL_Q},
    {"null-out", TFA_BF16, 1, 2, 2, 64, 64, 64, 0, M_NULL_OUT},
    {"null-aux", TFA_BF16, 1, 2, 2, 64, 64, 64, 0, M_NULL_AUX},
    {"misaligned-q", TFA_BF16, 1, 2, 2, 64, 64, 64, 0, M_MISALIGNED},
    {"misaligned-aux", TFA_BF16, 1, 2, 2, 64, 64, 64, 0, M_MISALIGNED_AUX},
    {"row-stride-below-d", TFA_BF16, 1, 2, 2, 64, 64, 64, 0, M_ROW_BELOW_D},
    {"negative-stride", TFA_BF16, 1, 2, 2, 64, 64, 64, 0, M_NEG_STRIDE},
    {"odd-stride", TFA_BF16, 1, 2, 2, 64, 64, 64, 0, M_ODD_STRIDE},
    {"scale-nan", TFA_BF16, 1, 2, 2, 64, 64, 64, 0, M_SCALE_NAN},
    {"scale-zero", TFA_BF16, 1, 2, 2, 64, 64, 64, 0, M_SCALE_ZERO},
    {"reserved-set", TFA_BF16, 1, 2, 2, 64, 64, 64, 0, M_RESERVED},
    {"bad-dtype", 7, 1, 2, 2, 64, 64, 64, 0, M_BAD_DTYPE},
    {"zero-b", TFA_BF16, 0, 2, 2, 64, 64, 64, 0, M_NONE},
    {"negative-h", TFA_BF16, 1, -2, 2, 64, 64, 64, 0, M_NONE},
    {"zero-hk", TFA_BF16, 1, 2, 0, 64, 64, 64, 0, M_NONE},
    {"h-not-multiple-of-hk", TFA_BF16, 1, 3, 2, 64, 64, 64, 0, M_NONE},
    {"zero-nq", TFA_BF16, 1, 2, 2, 0, 64, 64, 0, M_NONE},
    {"negative-nk", TFA_BF16, 1, 2, 2, 64, -64, 64, 0, M_NONE},
    {"int-min-nq", TFA_BF16, 1, 2, 2, INT_MIN, 64, 64, 1, M_NONE},
    {"d-zero", TFA_BF16, 1, 2, 2, 64, 64, 0, 0, M_NONE},
    {"d-negative", TFA_BF16, 1, 2, 2, 64, 64, -8, 0, M_NONE},
    {"d-12", TFA_BF16, 1, 2, 2, 64, 64, 12, 0, M_NONE},
    {"d-264", TFA_BF16, 1, 2, 2, 64, 64, 264, 0, M_NONE},
    {"d-int-max", TFA_BF16, 1, 2, 2, 64, 64, INT_MAX, 0, M_NONE},
    /* legal but extreme */
    {"nq-int-max", TFA_BF16, 1, 1, 1, INT_MAX, 64, 64, 1, M_NONE},
    {"nk-int-max", TFA_BF16, 1, 1, 1, 64, INT_MAX, 64, 1, M_NONE},
    {"nq-nk-int-max", TFA_F16, 1, 1, 1, INT_MAX, INT_MAX, 128, 0, M_NONE},
    {"nq-nk-int-max-d256", TFA_F16, 1, 1, 1, INT_MAX, INT_MAX, 256, 1, M_NONE},
    {"b-int-max", TFA_BF16, INT_MAX, 1, 1, 64, 64, 64, 0, M_NONE},
    {"h-int-max", TFA_BF16, 1, INT_MAX, 1, 1, 4096, 128, 0, M_NONE},
    {"b-h-int-max", TFA_BF16, INT_MAX, INT_MAX, INT_MAX, 1, 64, 64, 1, M_NONE},
    {"everything-int-max", TFA_BF16, INT_MAX, INT_MAX, INT_MAX, INT_MAX, INT_MAX, 256, 1, M_NONE},
    {"b-h-65536", TFA_BF16, 65536, 65536, 65536, 129, 129, 128, 1, M_NONE},
    {"b-h-nq-2^11-each", TFA_BF16, 2048, 2048, 2048, 2048, 2048, 128, 1, M_NONE},
    {"huge-strides", TFA_BF16, 2, 4, 2, 320, 385, 128, 1, M_HUGE_STRIDE},
    {"huge-strides-d256", TFA_F16, 2, 4, 4, 320, 385, 256, 0, M_HUGE_STRIDE},
    {"f32-nq-int-max", TFA_F32, 1, 1, 1, INT_MAX, INT_MAX, 72, 1, M_NONE},
};
#define NSHAPES ((int)(sizeof(SHAPES) / sizeof(SHAPES[0])))

static const int SPLITS[] = {-1, 0, 1, 2, 3, 4, 33, 4096, INT_MAX};
#define NSPLITS ((int)(sizeof(SPLITS) / sizeof(SPLITS[0])))
static const int WINDOWS[][2] = {{-1, -1}, {-1, 0}, {37, 20}, {0, 0}, {64, 33}, {-2, 0}, {INT_MAX, INT_MAX}, {INT_MAX, 0}, {INT_MIN, INT_MIN}};
#define NWINDOWS ((int)(sizeof(WINDOWS) / sizeof(WINDOWS[0])))

static void mutate_strides(int mut, int D, int64_t* q, int64_t* k) {
  if (mut == M_ROW_BELOW_D) k[2] = D - 8;
  if (mut == M_NEG_STRIDE) q[1] = -q[1];
  if (mut == M_ODD_STRIDE) k[0] += 3;
  if (mut == M_HUGE_STRIDE) {
    q[0] = INT64_MAX / 2 - 7, q[1] = INT64_MAX / 4 - 8;
    k[0] = (INT64_MAX / 2) & ~(int64_t)7, k[1] = (INT64_MAX / 4) & ~(int64_t)7, k[2] = ((int64_t)1 << 40);
  }
}

static void fill_fwd(tfa_fwd_params* p, const shape* s) {
  memset(p, 0, sizeof(*p));
  p->q = fake(1), p->k = fake(2), p->v = fake(3), p->out = fake(4), p->lse = (float*)fake(5);
  p->B = s->B, p->H = s->H, p->Hk = s->Hk, p->Nq = s->Nq, p->Nk = s->Nk, p->D = s->D;
  contig(p->q_stride, s->H, s->Nq, s->D), contig(p->o_stride, s->H, s->Nq, s->D);
  contig(p->k_stride, s->Hk, s->Nk, s->D), contig(p->v_stride, s->Hk, s->Nk, s->D);
  if (s->mut == M_BNHD) { /* (B,N,H,D) */
    p->q_stride[1] = p->o_stride[1] = s->D, p->q_stride[2] = p->o_stride[2] = (int64_t)s->H * s->D;
    p->k_stride[1] = p->v_stride[1] = s->D, p->k_stride[2] = p->v_stride[2] = (int64_t)s->Hk * s->D;
  }
  p->softmax_scale = 0.125f, p->is_causal = s->causal, p->dtype = s->dtype;
  p->out_dtype = (s->mut == M_OUT_F32 || s->dtype == TFA_F32) ? TFA_F32 : s->dtype;
  mutate_strides(s->mut, s->D, p->q_stride, p->k_stride);
  if (s->mut == M_NULL_Q) p->q = NULL;
  if (s->mut == M_NULL_OUT) p->out = NULL;
  if (s->mut == M_MISALIGNED) p->q = (char*)fake(1) + 2;
  if (s->mut == M_SCALE_NAN) p->softmax_scale = quiet_nan();
  if (s->mut == M_SCALE_ZERO) p->softmax_scale = 0.f;
  if (s->mut == M_RESERVED) p->reserved_ = 1;
  if (s->mut == M_FLAGS) p->flags = TFA_FWD_EXACT_MAX;
  if (s->mut == M_KV_OFFSET) p->kv_offset = 4096, p->nk_total = 8192;
}

static void walk_fwd(const shape* s) {
  tfa_fwd_params P;
  fill_fwd(&P, s);
  const tfa_fwd_params* p = s->mut == M_NULL_PARAMS ? NULL : &P;
  int g = 0, b = 0, l = 0;
  double fl = 0, by = 0;
  st("tfa_fwd_plan", tfa_fwd_plan(p, &g, &b, &l));
  st("tfa_fwd_plan(NULL outputs)", tfa_fwd_plan(p, NULL, NULL, NULL));
  cnt("tfa_fwd_variant", tfa_fwd_variant(p));
  cnt("tfa_fwd_rounding_rule", tfa_fwd_rounding_rule(p));
  st("tfa_fwd_work", tfa_fwd_work(p, &fl, &by));
  cnt("tfa_fwd_suggest_splits", tfa_fwd_suggest_splits(p));
  for (int i = 0; i < NSPLITS; ++i) cnt("tfa_fwd_splitkv_workspace", tfa_fwd_splitkv_workspace(p, SPLITS[i]));
  const float* slopes = s->mut == M_NULL_AUX ? NULL : (const float*)((char*)fake(6) + (s->mut == M_MISALIGNED_AUX ? 2 : 0));
  tfa_attn_bias bias;
  memset(&bias, 0, sizeof(bias));
  bias.bias = s->mut == M_NULL_AUX ? NULL : (char*)fake(7) + (s->mut == M_MISALIGNED_AUX ? 8 : 0);
  bias.dtype = s->dtype == TFA_F32 ? TFA_F32 : s->dtype;
  bias.stride[2] = s->mut == M_HUGE_STRIDE ? INT64_MAX / 2 - 7 : ((int64_t)(s->Nk > 0 ? s->Nk : 0) + 7) / 8 * 8;
  bias.stride[1] = smul(bias.stride[2], s->Nq > 0 ? s->Nq : 0);
  bias.stride[0] = smul(bias.stride[1], s->H > 0 ? s->H : 0);
  for (int w = 0; w < NWINDOWS; ++w) {
    const int wl = WINDOWS[w][0], wr = WINDOWS[w][1];
    const int64_t sbs = (w & 1) ? s->H : 0;
    st("tfa_fwd_local_plan", tfa_fwd_local_plan(p, wl, wr, &g, &b, &l));
    cnt("tfa_fwd_local_variant", tfa_fwd_local_variant(p, wl, wr));
    cnt("tfa_fwd_local_rounding_rule", tfa_fwd_local_rounding_rule(p, wl, wr));
    st("tfa_fwd_alibi_plan", tfa_fwd_alibi_plan(p, slopes, sbs, wl, wr, &g, &b, &l));
    cnt("tfa_fwd_alibi_variant", tfa_fwd_alibi_variant(p, slopes, sbs, wl, wr));
    cnt("tfa_fwd_alibi_rounding_rule", tfa_fwd_alibi_rounding_rule(p, slopes, sbs, wl, wr));
    st("tfa_fwd_softcap_plan", tfa_fwd_softcap_plan(p, w == 3 ? 0.f : 30.f, (w & 2) ? slopes : NULL, sbs, wl, wr, &g, &b, &l));
    cnt("tfa_fwd_softcap_variant", tfa_fwd_softcap_variant(p, 30.f, (w & 2) ? slopes : NULL, sbs, wl, wr));
    cnt("tfa_fwd_softcap_rounding_rule", tfa_fwd_softcap_rounding_rule(p, 3.0e38f, slopes, sbs, wl, wr));
    st("tfa_fwd_bias_plan", tfa_fwd_bias_plan(p, &bias, wl, wr, &g, &b, &l));
    cnt("tfa_fwd_bias_variant", tfa_fwd_bias_variant(p, &bias, wl, wr));
    cnt("tfa_fwd_bias_rounding_rule", tfa_fwd_bias_rounding_rule(p, w == 4 ? NULL : &bias, wl, wr));
  }
}

static void walk_bwd(const shape* s) {
  tfa_bwd_params P;
  memset(&P, 0, sizeof(P));
  P.q = fake(1), P.k = fake(2), P.v = fake(3), P.out = fake(4), P.dout = fake(5), P.lse = (const float*)fake(6);
  P.dq = fake(7), P.dk = fake(8), P.dv = fake(9), P.delta = (float*)fake(10);
  P.B = s->B, P.H = s->H, P.Hk = s->Hk, P.Nq = s->Nq, P.Nk = s->Nk, P.D = s->D;
  int64_t* qs[4] = {P.q_stride, P.o_stride, P.do_stride, P.dq_stride};
  int64_t* ks[4] = {P.k_stride, P.v_stride, P.dk_stride, P.dv_stride};
  for (int i = 0; i < 4; ++i) contig(qs[i], s->H, s->Nq, s->D), contig(ks[i], s->Hk, s->Nk, s->D);
  mutate_strides(s->mut, s->D, P.dq_stride, P.dk_stride);
  mutate_strides(s->mut == M_HUGE_STRIDE ? M_HUGE_STRIDE : M_NONE, s->D, P.q_stride, P.k_stride);
  P.softmax_scale = 0.125f, P.is_causal = s->causal, P.dtype = s->dtype, P.grad_dtype = s->mut == M_OUT_F32 ? TFA_F32 : s->dtype;
  if (s->mut == M_NULL_Q) P.q = NULL;
  if (s->mut == M_NULL_OUT) P.dv = NULL;
  if (s->mut == M_MISALIGNED) P.dout = (char*)fake(5) + 2;
  if (s->mut == M_SCALE_NAN) P.softmax_scale = quiet_nan();
  if (s->mut == M_SCALE_ZERO) P.softmax_scale = 0.f;
  if (s->mut == M_FLAGS) P.workspace = fake(11), P.workspace_bytes = INT64_MAX;
  const tfa_bwd_params* p = s->mut == M_NULL_PARAMS ? NULL : &P;
  double fl = 0, by = 0;
  st("tfa_bwd_plan", tfa_bwd_plan(p));
  cnt("tfa_bwd_workspace_bytes", tfa_bwd_workspace_bytes(p));
  st("tfa_bwd_work", tfa_bwd_work(p, &fl, &by));
  const float* slopes = s->mut == M_NULL_AUX ? NULL : (const float*)fake(12);
  tfa_attn_bias bias;
  memset(&bias, 0, sizeof(bias));
  bias.bias = fake(13), bias.dtype = TFA_F32, bias.stride[2] = ((int64_t)(s->Nk > 0 ? s->Nk : 0) + 7) / 8 * 8;
  for (int w = 0; w < NWINDOWS; ++w) {
    const int wl = WINDOWS[w][0], wr = WINDOWS[w][1];
    st("tfa_bwd_local_plan", tfa_bwd_local_plan(p, wl, wr));
    st("tfa_bwd_alibi_plan", tfa_bwd_alibi_plan(p, slopes, (w & 1) ? s->H : 0, wl, wr));
    st("tfa_bwd_softcap_plan", tfa_bwd_softcap_plan(p, w == 5 ? -1.f : 5.f, (w & 2) ? slopes : NULL, 0, wl, wr));
    st("tfa_bwd_bias_plan", tfa_bwd_bias_plan(p, &bias, wl, wr));
  }
}

static void walk_varlen(const shape* s) {
  /* the packed form of the same sizes: B sequences of at most Nq rows / Nk keys, totals that saturate at INT_MAX */
  tfa_varlen_fwd_params P;
  memset(&P, 0, sizeof(P));
  P.q = fake(1), P.k = fake(2), P.v = fake(3), P.out = fake(4), P.lse = (float*)fake(5);
  P.cu_seqlens_q = (const int32_t*)fake(6), P.cu_seqlens_k = (const int32_t*)fake(7);
  P.B = s->B, P.H = s->H, P.Hk = s->Hk, P.D = s->D, P.max_seqlen_q = s->Nq, P.max_seqlen_k = s->Nk;
  const int64_t tq = smul(s->B > 0 ? s->B : 0, s->Nq > 0 ? s->Nq : 0), tk = smul(s->B > 0 ? s->B : 0, s->Nk > 0 ? s->Nk : 0);
  P.total_q = s->Nq <= 0 ? s->Nq : (int32_t)(tq > INT_MAX ? INT_MAX : tq);
  P.total_k = s->Nk <= 0 ? s->Nk : (int32_t)(tk > INT_MAX ? INT_MAX : tk);
  P.q_stride[0] = P.o_stride[0] = s->D, P.q_stride[1] = P.o_stride[1] = smul(s->H > 0 ? s->H : 0, s->D);
  P.k_stride[0] = P.v_stride[0] = s->D, P.k_stride[1] = P.v_stride[1] = smul(s->Hk > 0 ? s->Hk : 0, s->D);
  if (s->mut == M_ROW_BELOW_D) P.k_stride[1] = s->D - 8;
  if (s->mut == M_NEG_STRIDE) P.q_stride[0] = -P.q_stride[0];
  if (s->mut == M_ODD_STRIDE) P.v_stride[1] += 3;
  if (s->mut == M_HUGE_STRIDE) P.q_stride[1] = INT64_MAX / 2 - 7, P.k_stride[1] = (INT64_MAX / 2) & ~(int64_t)7, P.k_stride[0] = (int64_t)1 << 40;
  P.softmax_scale = 0.125f, P.is_causal = s->causal, P.dtype = s->dtype, P.out_dtype = s->mut == M_OUT_F32 ? TFA_F32 : s->dtype;
  if (s->mut == M_NULL_Q) P.q = NULL;
  if (s->mut == M_NULL_OUT) P.out = NULL;
  if (s->mut == M_NULL_AUX) P.cu_seqlens_q = NULL;
  if (s->mut == M_MISALIGNED) P.q = (char*)fake(1) + 2;
  if (s->mut == M_MISALIGNED_AUX) P.cu_seqlens_k = (const int32_t*)((char*)fake(7) + 2);
  if (s->mut == M_SCALE_NAN) P.softmax_scale = quiet_nan();
  if (s->mut == M_SCALE_ZERO) P.softmax_scale = 0.f;
  if (s->mut == M_RESERVED) P.reserved_ = 1;
  if (s->mut == M_FLAGS) P.flags = TFA_FWD_EXACT_MAX;
  const tfa_varlen_fwd_params* p = s->mut == M_NULL_PARAMS ? NULL : &P;
  int g = 0, b = 0, l = 0;
  st("tfa_fwd_varlen_plan", tfa_fwd_varlen_plan(p, &g, &b, &l));
  cnt("tfa_fwd_varlen_variant", tfa_fwd_varlen_variant(p));
  cnt("tfa_fwd_varlen_rounding_rule", tfa_fwd_varlen_rounding_rule(p));
  const float* slopes = (const float*)fake(8);
  for (int w = 0; w < NWINDOWS; ++w) {
    const int wl = WINDOWS[w][0], wr = WINDOWS[w][1];
    st("tfa_fwd_varlen_local_plan", tfa_fwd_varlen_local_plan(p, wl, wr, &g, &b, &l));
    cnt("tfa_fwd_varlen_local_variant", tfa_fwd_varlen_local_variant(p, wl, wr));
    cnt("tfa_fwd_varlen_local_rounding_rule", tfa_fwd_varlen_local_rounding_rule(p, wl, wr));
    st("tfa_fwd_varlen_alibi_plan", tfa_fwd_varlen_alibi_plan(p, slopes, (w & 1) ? s->H : 0, wl, wr, &g, &b, &l));
    cnt("tfa_fwd_varlen_alibi_variant", tfa_fwd_varlen_alibi_variant(p, slopes, 0, wl, wr));
    cnt("tfa_fwd_varlen_alibi_rounding_rule", tfa_fwd_varlen_alibi_rounding_rule(p, slopes, 0, wl, wr));
    st("tfa_fwd_varlen_softcap_plan", tfa_fwd_varlen_softcap_plan(p, 30.f, (w & 2) ? slopes : NULL, 0, wl, wr, &g, &b, &l));
    cnt("tfa_fwd_varlen_softcap_variant", tfa_fwd_varlen_softcap_variant(p, 30.f, NULL, 0, wl, wr));
    cnt("tfa_fwd_varlen_softcap_rounding_rule", tfa_fwd_varlen_softcap_rounding_rule(p, 30.f, NULL, 0, wl, wr));
  }
  /* its paged form: pages of 64, 256 and 2^20 keys; tables of INT_MAX blocks and pools of INT_MAX pages */
  static const int PG[][3] = {{64, 8, 64}, {256, 2, 19}, {96, 8, 64}, {0, 8, 64}, {64, 0, 64}, {64, 8, 0}, {1 << 20, INT_MAX, INT_MAX}, {INT_MAX / 64 * 64, INT_MAX, INT_MAX},
                              {256, 1 << 24, 1 << 24}};
  for (int i = 0; i < (int)(sizeof(PG) / sizeof(PG[0])); ++i) {
    tfa_paged_kv pg;
    memset(&pg, 0, sizeof(pg));
    pg.block_table = s->mut == M_NULL_AUX ? NULL : (const int32_t*)((char*)fake(9) + (s->mut == M_MISALIGNED_AUX ? 2 : 0));
    pg.page_size = PG[i][0], pg.max_blocks = PG[i][1], pg.num_pages = PG[i][2], pg.table_stride = PG[i][1];
    pg.k_page_stride = pg.v_page_stride = s->mut == M_HUGE_STRIDE ? (INT64_MAX / 2) & ~(int64_t)7 : smul(smul(PG[i][0], s->Hk > 0 ? s->Hk : 0), s->D > 0 ? s->D : 0);
    if (s->mut == M_RESERVED) pg.reserved_ = 1;
    if (s->mut == M_NEG_STRIDE) pg.table_stride = -1;
    st("tfa_fwd_varlen_paged_plan", tfa_fwd_varlen_paged_plan(p, i == 4 && s->mut == M_NULL_AUX ? NULL : &pg, &g, &b, &l));
    cnt("tfa_fwd_varlen_paged_variant", tfa_fwd_varlen_paged_variant(p, &pg));
    cnt("tfa_fwd_varlen_paged_rounding_rule", tfa_fwd_varlen_paged_rounding_rule(p, &pg));
  }
  /* ... and the packed backward's plans */
  tfa_varlen_bwd_params Q;
  memset(&Q, 0, sizeof(Q));
  Q.q = P.q, Q.k = P.k, Q.v = P.v, Q.out = fake(4), Q.dout = fake(10), Q.lse = (const float*)fake(5), Q.dq = fake(11), Q.dk = fake(12), Q.dv = fake(13);
  Q.delta = (float*)fake(14), Q.cu_seqlens_q = P.cu_seqlens_q, Q.cu_seqlens_k = P.cu_seqlens_k;
  Q.B = P.B, Q.H = P.H, Q.Hk = P.Hk, Q.D = P.D, Q.max_seqlen_q = P.max_seqlen_q, Q.max_seqlen_k = P.max_seqlen_k, Q.total_q = P.total_q, Q.total_k = P.total_k;
  int64_t* qs[4] = {Q.q_stride, Q.o_stride, Q.do_stride, Q.dq_stride};
  int64_t* ks[4] = {Q.k_stride, Q.v_stride, Q.dk_stride, Q.dv_stride};
  for (int i = 0; i < 4; ++i) qs[i][0] = P.q_stride[0], qs[i][1] = P.q_stride[1], ks[i][0] = P.k_stride[0], ks[i][1] = P.k_stride[1];
  Q.softmax_scale = P.softmax_scale, Q.is_causal = P.is_causal, Q.dtype = P.dtype, Q.grad_dtype = P.out_dtype, Q.flags = P.flags, Q.reserved_ = P.reserved_;
  const tfa_varlen_bwd_params* q = s->mut == M_NULL_PARAMS ? NULL : &Q;
  for (int w = 0; w < NWINDOWS; ++w) {
    const int wl = WINDOWS[w][0], wr = WINDOWS[w][1];
    st("tfa_bwd_varlen_local_plan", tfa_bwd_varlen_local_plan(q, wl, wr));
    st("tfa_bwd_varlen_alibi_plan", tfa_bwd_varlen_alibi_plan(q, slopes, (w & 1) ? s->H : 0, wl, wr));
    st("tfa_bwd_varlen_softcap_plan", tfa_bwd_varlen_softcap_plan(q, 5.f, (w & 2) ? slopes : NULL, 0, wl, wr));
  }
}

/* ---- the K/V-cache family ----------------------------------------------------------------------------------------------------------------------- */
typedef struct kvshape { const char* name; int dtype, B, H, Hk, Nq, D, capacity, page, num_pages, n_new, causal, max_q, total_q, mut; } kvshape;
static const kvshape KV[] = {
    {"decode-contig", TFA_BF16, 4, 8, 2, 1, 128, 4096, 0, 0, 0, 1, 1, 4, M_NONE},
    {"decode-paged", TFA_F16, 4, 8, 2, 1, 64, 4096, 256, 70, 0, 1, 1, 4, M_NONE},
    {"append-paged", TFA_BF16, 3, 4, 1, 5, 128, 1024, 64, 51, 5, 1, 5, 15, M_NONE},
    {"prefill-chunks", TFA_BF16, 5, 8, 2, 33, 96, 2048, 256, 43, 0, 1, 300, 450, M_NONE},
    {"mha-d16", TFA_F16, 2, 3, 3, 7, 16, 640, 64, 23, 0, 0, 7, 14, M_NONE},
    {"tree-70-rows", TFA_BF16, 2, 8, 2, 70, 128, 1024, 256, 11, 70, 1, 70, 140, M_NONE},
    {"null-params", TFA_BF16, 4, 8, 2, 1, 128, 4096, 0, 0, 0, 1, 1, 4, M_NULL_PARAMS},
    {"null-q", TFA_BF16, 4, 8, 2, 1, 128, 4096, 0, 0, 0, 1, 1, 4, M_NULL_Q},
    {"null-out", TFA_BF16, 4, 8, 2, 1, 128, 4096, 0, 0, 0, 1, 1, 4, M_NULL_OUT},
    {"null-aux", TFA_BF16, 4, 8, 2, 1, 128, 4096, 256, 70, 0, 1, 1, 4, M_NULL_AUX},
    {"misaligned-q", TFA_BF16, 4, 8, 2, 1, 128, 4096, 0, 0, 0, 1, 1, 4, M_MISALIGNED},
    {"misaligned-aux", TFA_BF16, 4, 8, 2, 1, 128, 4096, 256, 70, 0, 1, 1, 4, M_MISALIGNED_AUX},
    {"row-stride-below-d", TFA_BF16, 4, 8, 2, 1, 128, 4096, 0, 0, 0, 1, 1, 4, M_ROW_BELOW_D},
    {"negative-stride", TFA_BF16, 4, 8, 2, 1, 128, 4096, 0, 0, 0, 1, 1, 4, M_NEG_STRIDE},
    {"odd-stride", TFA_BF16, 4, 8, 2, 1, 128, 4096, 0, 0, 0, 1, 1, 4, M_ODD_STRIDE},
    {"scale-nan", TFA_BF16, 4, 8, 2, 1, 128, 4096, 0, 0, 0, 1, 1, 4, M_SCALE_NAN},
    {"reserved-set", TFA_BF16, 4, 8, 2, 1, 128, 4096, 0, 0, 0, 1, 1, 4, M_RESERVED},
    {"bad-dtype", TFA_F32, 4, 8, 2, 1, 128, 4096, 0, 0, 0, 1, 1, 4, M_NONE},
    {"zero-b", TFA_BF16, 0, 8, 2, 1, 128, 4096, 0, 0, 0, 1, 1, 4, M_NONE},
    {"negative-capacity", TFA_BF16, 4, 8, 2, 1, 128, -4096, 256, 70, 0, 1, 1, 4, M_NONE},
    {"page-96", TFA_BF16, 4, 8, 2, 1, 128, 4096, 96, 70, 0, 1, 1, 4, M_NONE},
    {"capacity-not-pages", TFA_BF16, 4, 8, 2, 1, 128, 4000, 256, 70, 0, 1, 1, 4, M_NONE},
    {"zero-pages", TFA_BF16, 4, 8, 2, 1, 128, 4096, 256, 0, 0, 1, 1, 4, M_NONE},
    {"negative-n-new", TFA_BF16, 4, 8, 2, 1, 128, 4096, 0, 0, -1, 1, 1, 4, M_NONE},
    {"d-136", TFA_BF16, 4, 8, 2, 1, 136, 4096, 0, 0, 0, 1, 1, 4, M_NONE},
    {"zero-max-q", TFA_BF16, 4, 8, 2, 1, 128, 4096, 0, 0, 0, 1, 0, 0, M_NONE},
    {"negative-total-q", TFA_BF16, 4, 8, 2, 1, 128, 4096, 0, 0, 0, 1, 1, -4, M_NONE},
    /* legal but extreme */
    {"capacity-2^30-pages-2^16", TFA_BF16, 4, 8, 2, 1, 128, 1 << 30, 1 << 16, INT_MAX, 0, 1, 1, 4, M_NONE},
    {"capacity-page-int-max", TFA_F16, 2, 8, 2, 1, 64, INT_MAX / 64 * 64, INT_MAX / 64 * 64, INT_MAX, 0, 1, 1, 2, M_NONE},
    {"capacity-int-max-contig", TFA_BF16, 1, 8, 8, 1, 128, INT_MAX, 0, 0, 0, 0, 1, 1, M_NONE},
    {"capacity-2^30-page-64", TFA_BF16, 8, 64, 8, 1, 128, 1 << 30, 64, INT_MAX, 0, 1, 1, 8, M_NONE},
    {"b-h-nq-int-max", TFA_BF16, INT_MAX, INT_MAX, INT_MAX, INT_MAX, 128, 4096, 0, 0, 0, 1, INT_MAX, INT_MAX, M_NONE},
    {"b-h-65536", TFA_BF16, 65536, 65536, 1, 1, 128, 4096, 256, 70, 0, 1, 1, 65536, M_NONE},
    {"max-q-total-q-int-max", TFA_BF16, 4, 8, 2, 1, 128, 1 << 20, 256, 1 << 14, 0, 1, INT_MAX, INT_MAX, M_NONE},
    {"total-q-int-max-g128", TFA_F16, INT_MAX / 2, 128, 1, 1, 64, 4096, 0, 0, 0, 1, INT_MAX - 1, INT_MAX, M_NONE},
    {"total-q-int-max-not-causal", TFA_F16, INT_MAX, 4, 4, 1, 64, 4096, 0, 0, 0, 0, INT_MAX, INT_MAX, M_NONE},
    {"nq-int-max-n-new-int-max", TFA_BF16, 2, 4, 2, INT_MAX, 128, 1 << 20, 0, 0, INT_MAX, 1, INT_MAX, INT_MAX, M_NONE},
    {"huge-strides", TFA_BF16, 4, 8, 2, 3, 128, 4096, 256, 70, 0, 1, 3, 12, M_HUGE_STRIDE},
    {"huge-strides-contig", TFA_BF16, 4, 8, 2, 3, 128, 4096, 0, 0, 0, 1, 3, 12, M_HUGE_STRIDE},
};
#define NKV ((int)(sizeof(KV) / sizeof(KV[0])))

static void fill_kv(tfa_kvcache_params* p, const kvshape* s, int packed_q) {
  memset(p, 0, sizeof(*p));
  p->q = fake(1), p->out = fake(2), p->lse = (float*)fake(3), p->k_cache = fake(4), p->v_cache = fake(5), p->cache_seqlens = (const int32_t*)fake(6);
  p->block_table = s->page ? (const int32_t*)fake(7) : NULL;
  if (s->n_new && !packed_q) p->k_new = fake(8), p->v_new = fake(9);
  p->B = s->B, p->H = s->H, p->Hk = s->Hk, p->Nq = s->Nq, p->D = s->D, p->capacity = s->capacity, p->n_new = packed_q ? 0 : s->n_new;
  p->page_size = s->page, p->num_pages = s->num_pages;
  const int64_t H = s->H > 0 ? s->H : 0, Hk = s->Hk > 0 ? s->Hk : 0, D = s->D > 0 ? s->D : 0, rows = packed_q ? (s->total_q > 0 ? s->total_q : 0) : (s->Nq > 0 ? s->Nq : 0);
  if (packed_q) { /* q (total_q, H, D); out the contiguous (H, total_q, D) a merge writes */
    p->q_stride[1] = D, p->q_stride[2] = smul(H, D), p->o_stride[1] = smul(rows, D), p->o_stride[2] = D;
  } else { /* q (B, Nq, H, D); out the contiguous (B, H, Nq, D) */
    p->q_stride[0] = smul(smul(rows, H), D), p->q_stride[1] = D, p->q_stride[2] = smul(H, D);
    contig(p->o_stride, H, rows, D);
  }
  const int64_t slab = s->page ? s->page : (s->capacity > 0 ? s->capacity : 0);
  p->k_stride[0] = p->v_stride[0] = smul(smul(slab, Hk), D), p->k_stride[1] = p->v_stride[1] = D, p->k_stride[2] = p->v_stride[2] = smul(Hk, D);
  const int64_t nn = s->n_new > 0 ? s->n_new : 0;
  p->knew_stride[0] = p->vnew_stride[0] = smul(smul(nn, Hk), D), p->knew_stride[1] = p->vnew_stride[1] = D, p->knew_stride[2] = p->vnew_stride[2] = smul(Hk, D);
  p->block_table_stride = s->page > 0 && s->capacity > 0 ? s->capacity / s->page : 0;
  p->softmax_scale = 0.088f, p->is_causal = s->causal, p->dtype = s->dtype;
  if (s->mut == M_NULL_Q) p->q = NULL;
  if (s->mut == M_NULL_OUT) p->out = NULL;
  if (s->mut == M_NULL_AUX) p->cache_seqlens = NULL;
  if (s->mut == M_MISALIGNED) p->q = (char*)fake(1) + 2;
  if (s->mut == M_MISALIGNED_AUX) p->block_table = (const int32_t*)((char*)fake(7) + 2);
  if (s->mut == M_ROW_BELOW_D) p->k_stride[2] = D - 8;
  if (s->mut == M_NEG_STRIDE) p->v_stride[0] = -p->v_stride[0];
  if (s->mut == M_ODD_STRIDE) p->q_stride[2] += 3;
  if (s->mut == M_HUGE_STRIDE) {
    p->k_stride[0] = p->v_stride[0] = (INT64_MAX / 2) & ~(int64_t)15, p->q_stride[2] = (INT64_MAX / 2) & ~(int64_t)15, p->q_stride[1] = (int64_t)1 << 50;
    p->block_table_stride = INT64_MAX / 2;
  }
  if (s->mut == M_SCALE_NAN) p->softmax_scale = quiet_nan();
  if (s->mut == M_RESERVED) p->reserved2_ = 1;
}

static void walk_kv(const kvshape* s) {
  tfa_kvcache_params P4, PQ;
  fill_kv(&P4, s, 0);
  fill_kv(&PQ, s, 1);
  const tfa_kvcache_params* p4 = s->mut == M_NULL_PARAMS ? NULL : &P4;
  const tfa_kvcache_params* pq = s->mut == M_NULL_PARAMS ? NULL : &PQ;
  tfa_kvcache_fp8 q8;
  memset(&q8, 0, sizeof(q8));
  q8.k_descale = (const float*)fake(10), q8.v_descale = (const float*)((char*)fake(11) + (s->mut == M_MISALIGNED_AUX ? 2 : 0));
  q8.k_descale_stride[0] = s->Hk > 0 ? s->Hk : 0, q8.k_descale_stride[1] = 1, q8.format = TFA_KV_E4M3;
  if (s->mut == M_NEG_STRIDE) q8.v_descale_stride[0] = -1;
  if (s->mut == M_HUGE_STRIDE) q8.k_descale_stride[0] = INT64_MAX / 2;
  if (s->mut == M_RESERVED) q8.reserved_ = 1;
  tfa_kvcache_varlen_q vq;
  memset(&vq, 0, sizeof(vq));
  vq.cu_seqlens_q = s->mut == M_NULL_AUX ? NULL : (const int32_t*)((char*)fake(12) + (s->mut == M_MISALIGNED_AUX ? 2 : 0));
  vq.max_seqlen_q = s->max_q, vq.total_q = s->total_q;
  if (s->mut == M_RESERVED) vq.reserved_[1] = 1;
  tfa_kvcache_tree tree;
  memset(&tree, 0, sizeof(tree));
  tree.mask = s->mut == M_NULL_AUX ? NULL : (char*)fake(13) + (s->mut == M_MISALIGNED_AUX ? 4 : 0);
  tree.batch_stride = s->mut == M_HUGE_STRIDE ? INT64_MAX / 2 : (s->Nq > 0 ? s->Nq : 0), tree.row_stride = s->mut == M_NEG_STRIDE ? -1 : 1;
  int g = 0, b = 0, l = 0;
  cnt("tfa_fwd_kvcache_suggest_splits", tfa_fwd_kvcache_suggest_splits(p4));
  for (int pk = -1; pk <= 3; ++pk) {
    cnt("tfa_fwd_kvcache_pack_suggest_splits", tfa_fwd_kvcache_pack_suggest_splits(p4, pk));
    cnt("tfa_fwd_kvcache_varlen_suggest_splits", tfa_fwd_kvcache_varlen_suggest_splits(pq, &vq, pk));
    for (int causal = 0; causal <= 1; ++causal) {
      cnt("tfa_kvcache_varlen_schedule_size", tfa_kvcache_varlen_schedule_size(pq, &vq, pk, causal));
      st("tfa_kvcache_varlen_schedule_plan", tfa_kvcache_varlen_schedule_plan(pq, &vq, pk, causal, &g, &b, &l));
    }
  }
  cnt("tfa_kvcache_varlen_schedule_size(NULL vq)", tfa_kvcache_varlen_schedule_size(pq, NULL, TFA_PACK_GQA_AUTO, 1));
  static const int WL[] = {-1, 0, 63, 4096, INT_MAX};
  for (int w = 0; w < 5; ++w) {
    cnt("tfa_fwd_kvcache_window_suggest_splits", tfa_fwd_kvcache_window_suggest_splits(p4, NULL, TFA_PACK_GQA_AUTO, WL[w]));
    cnt("tfa_fwd_kvcache_window_suggest_splits(vq)", tfa_fwd_kvcache_window_suggest_splits(pq, &vq, TFA_PACK_GQA_ON, WL[w]));
  }
  cnt("tfa_fwd_kvcache_tree_suggest_splits", tfa_fwd_kvcache_tree_suggest_splits(p4, NULL, TFA_PACK_GQA_AUTO, &tree));
  cnt("tfa_fwd_kvcache_tree_suggest_splits(vq)", tfa_fwd_kvcache_tree_suggest_splits(pq, &vq, TFA_PACK_GQA_AUTO, &tree));
  for (int i = 0; i < NSPLITS; ++i) {
    const int sp = SPLITS[i];
    const tfa_kvcache_fp8* f8 = (i & 1) ? &q8 : NULL;
    const int pk = i % 3;
    st("tfa_fwd_kvcache_plan", tfa_fwd_kvcache_plan(p4, sp, &g, &b, &l));
    cnt("tfa_fwd_kvcache_workspace", tfa_fwd_kvcache_workspace(p4, sp));
    st("tfa_fwd_kvcache_fp8_plan", tfa_fwd_kvcache_fp8_plan(p4, &q8, sp, &g, &b, &l));
    cnt("tfa_fwd_kvcache_fp8_workspace", tfa_fwd_kvcache_fp8_workspace(p4, i == 2 ? NULL : &q8, sp));
    st("tfa_fwd_kvcache_pack_plan", tfa_fwd_kvcache_pack_plan(p4, f8, pk, sp, &g, &b, &l));
    cnt("tfa_fwd_kvcache_pack_workspace", tfa_fwd_kvcache_pack_workspace(p4, f8, pk, sp));
    st("tfa_fwd_kvcache_varlen_plan", tfa_fwd_kvcache_varlen_plan(pq, &vq, f8, pk, sp, &g, &b, &l));
    cnt("tfa_fwd_kvcache_varlen_workspace", tfa_fwd_kvcache_varlen_workspace(pq, &vq, f8, pk, sp));
    st("tfa_fwd_kvcache_varlen_sched_plan", tfa_fwd_kvcache_varlen_sched_plan(pq, &vq, f8, pk, sp, &g, &b, &l));
    for (int w = 0; w < 5; w += 2) {
      st("tfa_fwd_kvcache_window_plan", tfa_fwd_kvcache_window_plan(p4, NULL, f8, pk, WL[w], sp, 0, &g, &b, &l));
      st("tfa_fwd_kvcache_window_plan(vq)", tfa_fwd_kvcache_window_plan(pq, &vq, f8, pk, WL[w], sp, i & 1, &g, &b, &l));
      cnt("tfa_fwd_kvcache_window_workspace", tfa_fwd_kvcache_window_workspace(p4, NULL, f8, pk, WL[w], sp));
      cnt("tfa_fwd_kvcache_window_workspace(vq)", tfa_fwd_kvcache_window_workspace(pq, &vq, f8, pk, WL[w], sp));
    }
    st("tfa_fwd_kvcache_window_plan(sched, no vq)", tfa_fwd_kvcache_window_plan(p4, NULL, f8, pk, 63, sp, 1, &g, &b, &l));
    st("tfa_fwd_kvcache_tree_plan", tfa_fwd_kvcache_tree_plan(p4, NULL, f8, pk, &tree, sp, 0, &g, &b, &l));
    st("tfa_fwd_kvcache_tree_plan(vq)", tfa_fwd_kvcache_tree_plan(pq, &vq, f8, pk, i == 3 ? NULL : &tree, sp, i & 1, &g, &b, &l));
    cnt("tfa_fwd_kvcache_tree_workspace", tfa_fwd_kvcache_tree_workspace(p4, NULL, f8, pk, &tree, sp));
    cnt("tfa_fwd_kvcache_tree_workspace(vq)", tfa_fwd_kvcache_tree_workspace(pq, &vq, f8, pk, &tree, sp));
  }
  /* the packed append of the same batch (total_new = total_q rows), plain, into e4m3 and with q */
  tfa_kvcache_append_varlen_params A;
  memset(&A, 0, sizeof(A));
  A.k = fake(14), A.v = fake(15), A.k_cache = fake(4), A.v_cache = fake(5), A.cu_seqlens = vq.cu_seqlens_q, A.cache_seqlens = PQ.cache_seqlens;
  A.block_table = PQ.block_table, A.rotary_cos = fake(16), A.rotary_sin = s->mut == M_NULL_OUT ? NULL : fake(17);
  A.B = s->B, A.total_new = s->total_q, A.Hk = s->Hk, A.D = s->D, A.capacity = s->capacity, A.page_size = s->page, A.num_pages = s->num_pages;
  A.rotary_dim = s->D >= 32 ? 32 : s->D, A.seqlen_ro = s->capacity, A.rotary_interleaved = s->mut == M_RESERVED ? 2 : (s->B & 1), A.dtype = s->dtype, A.cs_dtype = TFA_F32;
  A.k_stride[0] = A.v_stride[0] = PQ.k_stride[1], A.k_stride[1] = A.v_stride[1] = PQ.k_stride[2];
  for (int i = 0; i < 3; ++i) A.kc_stride[i] = PQ.k_stride[i], A.vc_stride[i] = PQ.v_stride[i];
  A.block_table_stride = PQ.block_table_stride, A.cos_stride = A.sin_stride = s->mut == M_HUGE_STRIDE ? INT64_MAX / 2 - 3 : 16;
  if (s->mut == M_NULL_Q) A.k = NULL;
  if (s->mut == M_MISALIGNED) A.v = (char*)fake(15) + 2;
  tfa_append_q rq;
  memset(&rq, 0, sizeof(rq));
  rq.q = s->mut == M_NULL_AUX ? NULL : fake(1), rq.H = s->H, rq.q_stride[0] = PQ.q_stride[1], rq.q_stride[1] = PQ.q_stride[2];
  const tfa_kvcache_append_varlen_params* a = s->mut == M_NULL_PARAMS ? NULL : &A;
  st("tfa_kvcache_append_varlen_plan", tfa_kvcache_append_varlen_plan(a, &g, &b));
  st("tfa_kvcache_append_varlen_plan(NULL outputs)", tfa_kvcache_append_varlen_plan(a, NULL, NULL));
  st("tfa_kvcache_append_varlen_ex_plan", tfa_kvcache_append_varlen_ex_plan(a, NULL, NULL, &g, &b));
  st("tfa_kvcache_append_varlen_ex_plan(q8)", tfa_kvcache_append_varlen_ex_plan(a, &q8, NULL, &g, &b));
  st("tfa_kvcache_append_varlen_ex_plan(rq)", tfa_kvcache_append_varlen_ex_plan(a, NULL, &rq, &g, &b));
  st("tfa_kvcache_append_varlen_ex_plan(q8, rq)", tfa_kvcache_append_varlen_ex_plan(a, &q8, &rq, &g, &b));
  A.rotary_cos = A.rotary_sin = NULL;
  st("tfa_kvcache_append_varlen_plan(no tables)", tfa_kvcache_append_varlen_plan(a, &g, &b));
  st("tfa_kvcache_append_varlen_ex_plan(rq, no tables)", tfa_kvcache_append_varlen_ex_plan(a, NULL, &rq, &g, &b));
}

/* ---- rotary ------------------------------------------------------------------------------------------------------------------------------------- */
typedef struct roshape { const char* name; int dtype, B, N, H, H2, D, rd, ro, packed, mut; } roshape;
static const roshape RO[] = {
    {"b2-n5", TFA_BF16, 2, 5, 3, 0, 64, 64, 80, 0, M_NONE},
    {"pair-d128-rd32", TFA_F16, 2, 70, 3, 1, 128, 32, 80, 0, M_NONE},
    {"packed-d40-rd16", TFA_F16, 4, 76, 3, 1, 40, 16, 80, 1, M_NONE},
    {"null-params", TFA_BF16, 2, 5, 3, 0, 64, 64, 80, 0, M_NULL_PARAMS},
    {"null-x", TFA_BF16, 2, 5, 3, 0, 64, 64, 80, 0, M_NULL_Q},
    {"null-cos", TFA_BF16, 2, 5, 3, 0, 64, 64, 80, 0, M_NULL_AUX},
    {"x2-without-out2", TFA_BF16, 2, 5, 3, 1, 64, 64, 80, 0, M_NULL_OUT},
    {"misaligned-x", TFA_BF16, 2, 5, 3, 0, 64, 64, 80, 0, M_MISALIGNED},
    {"misaligned-cu", TFA_BF16, 2, 5, 3, 0, 64, 64, 80, 1, M_MISALIGNED_AUX},
    {"negative-stride", TFA_BF16, 2, 5, 3, 0, 64, 64, 80, 0, M_NEG_STRIDE},
    {"odd-stride", TFA_BF16, 2, 5, 3, 0, 64, 64, 80, 0, M_ODD_STRIDE},
    {"table-row-below-rd/2", TFA_BF16, 2, 5, 3, 0, 64, 64, 80, 0, M_ROW_BELOW_D},
    {"bad-dtype", TFA_F32, 2, 5, 3, 0, 64, 64, 80, 0, M_NONE},
    {"rd-24", TFA_BF16, 2, 5, 3, 0, 64, 24, 80, 0, M_NONE},
    {"rd-above-d", TFA_BF16, 2, 5, 3, 0, 64, 80, 80, 0, M_NONE},
    {"d-12", TFA_BF16, 2, 5, 3, 0, 12, 16, 80, 0, M_NONE},
    {"zero-n", TFA_BF16, 2, 0, 3, 0, 64, 64, 80, 0, M_NONE},
    {"negative-h2", TFA_BF16, 2, 5, 3, -1, 64, 64, 80, 0, M_NONE},
    {"interleaved-2", TFA_BF16, 2, 5, 3, 0, 64, 64, 80, 0, M_RESERVED},
    {"n-int-max", TFA_BF16, 1, INT_MAX, 1, 0, 16, 16, INT_MAX, 1, M_NONE},
    {"b-n-h-int-max", TFA_BF16, INT_MAX, INT_MAX, INT_MAX, INT_MAX, 64, 64, INT_MAX, 0, M_NONE},
    {"b-n-65536-h-h2-2^30", TFA_F16, 65536, 65536, 1 << 30, 1 << 30, 256, 256, 80, 0, M_NONE},
    {"d-rd-int-max", TFA_F16, 2, 5, 3, 0, INT_MAX / 16 * 16, INT_MAX / 16 * 16, 80, 0, M_NONE},
    {"grid-just-below-2^31", TFA_BF16, 1, (1 << 27) - 1, 1024, 0, 32, 32, 80, 1, M_NONE},
    {"huge-strides", TFA_BF16, 2, 5, 3, 1, 64, 64, 80, 0, M_HUGE_STRIDE},
};
#define NRO ((int)(sizeof(RO) / sizeof(RO[0])))

static void walk_rotary(const roshape* s) {
  tfa_rotary_params P;
  memset(&P, 0, sizeof(P));
  P.x = fake(1), P.out = fake(2), P.cos = fake(5), P.sin = fake(6), P.seqlen_offsets = (const int32_t*)fake(7);
  if (s->H2 != 0) P.x2 = fake(3), P.out2 = fake(4);
  if (s->packed) P.cu_seqlens = (const int32_t*)((char*)fake(8) + (s->mut == M_MISALIGNED_AUX ? 2 : 0));
  P.B = s->B, P.N = s->N, P.H = s->H, P.H2 = s->H2, P.D = s->D, P.rotary_dim = s->rd, P.seqlen_ro = s->ro, P.seqlen_offset = s->mut == M_HUGE_STRIDE ? INT_MAX : 7;
  const int64_t N = s->N > 0 ? s->N : 0, H = s->H > 0 ? s->H : 0, H2 = s->H2 > 0 ? s->H2 : 0, D = s->D > 0 ? s->D : 0;
  P.x_stride[0] = P.o_stride[0] = smul(smul(N, H), D), P.x_stride[1] = P.o_stride[1] = D, P.x_stride[2] = P.o_stride[2] = smul(H, D);
  P.x2_stride[0] = P.o2_stride[0] = smul(smul(N, H2), D), P.x2_stride[1] = P.o2_stride[1] = D, P.x2_stride[2] = P.o2_stride[2] = smul(H2, D);
  P.cos_stride = P.sin_stride = s->mut == M_ROW_BELOW_D ? 8 : (s->rd > 0 ? (s->rd / 2 + 7) / 8 * 8 : 8);
  P.dtype = s->dtype, P.cs_dtype = s->dtype, P.interleaved = s->mut == M_RESERVED ? 2 : (s->N & 1);
  if (s->mut == M_NULL_Q) P.x = NULL;
  if (s->mut == M_NULL_AUX) P.cos = NULL;
  if (s->mut == M_NULL_OUT) P.out2 = NULL;
  if (s->mut == M_MISALIGNED) P.x = (char*)fake(1) + 2;
  if (s->mut == M_NEG_STRIDE) P.o_stride[2] = -P.o_stride[2];
  if (s->mut == M_ODD_STRIDE) P.x_stride[1] += 4;
  if (s->mut == M_HUGE_STRIDE) {
    P.x_stride[0] = (INT64_MAX / 2) & ~(int64_t)7, P.x_stride[2] = (INT64_MAX / 4) & ~(int64_t)7, P.o2_stride[1] = (int64_t)1 << 60;
    P.cos_stride = (INT64_MAX / 2) & ~(int64_t)7;
  }
  int g = 0, b = 0;
  st("tfa_rotary_plan", tfa_rotary_plan(s->mut == M_NULL_PARAMS ? NULL : &P, &g, &b));
  st("tfa_rotary_plan(NULL outputs)", tfa_rotary_plan(s->mut == M_NULL_PARAMS ? NULL : &P, NULL, NULL));
}

static int plan_mode(void) {
  char name[64];
  printf("tfa_version %d, %d kernel variants\n", tfa_version(), tfa_num_variants());
  for (int v = -2; v <= tfa_num_variants(); ++v) {
    const char* vn = tfa_variant_name(v);
    printf("variant %d: available %d, name %s\n", v, tfa_variant_available(v), vn ? vn : "(null)");
  }
  for (int s = TFA_ERR_SCALE - 1; s <= 1; ++s) printf("tfa_strerror(%d) = %s\n", s, tfa_strerror(s));
  set_row("library", "knobs");
  st("tfa_get_variant + 1", tfa_get_variant() + 1);
  /* every variant number, forced, through the plans of four shapes; then numbers outside the table */
  for (int v = 0; v < tfa_num_variants(); ++v) {
    const int set = tfa_set_variant(v);
    snprintf(name, sizeof(name), "%d", v);
    set_row("forced variant", name);
    st("tfa_set_variant", set);
    if (set != TFA_OK) continue;
    for (int i = 1; i <= 4; ++i) {
      tfa_fwd_params P;
      fill_fwd(&P, &SHAPES[i]);
      int g = 0, b = 0, l = 0;
      st("tfa_fwd_plan", tfa_fwd_plan(&P, &g, &b, &l));
      cnt("tfa_fwd_variant", tfa_fwd_variant(&P));
      cnt("tfa_fwd_rounding_rule", tfa_fwd_rounding_rule(&P));
    }
  }
  set_row("forced variant", "out of range");
  st("tfa_set_variant(INT_MAX)", tfa_set_variant(INT_MAX));
  st("tfa_set_variant(INT_MIN)", tfa_set_variant(INT_MIN));
  st("tfa_set_variant(-1)", tfa_set_variant(-1));
  for (int i = 0; i < NSHAPES; ++i) {
    set_row("fwd", SHAPES[i].name);
    walk_fwd(&SHAPES[i]);
    set_row("bwd", SHAPES[i].name);
    walk_bwd(&SHAPES[i]);
    set_row("varlen", SHAPES[i].name);
    walk_varlen(&SHAPES[i]);
  }
  for (int i = 0; i < NKV; ++i) {
    set_row("kvcache", KV[i].name);
    walk_kv(&KV[i]);
  }
  for (int i = 0; i < NRO; ++i) {
    set_row("rotary", RO[i].name);
    walk_rotary(&RO[i]);
  }
  flush_row();
  printf("%d calls, %d answers that are neither a success nor a tfa_status\n", g_calls, g_bad);
  return g_bad ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && strcmp(argv[1], "run") == 0) return run_mode(argv[2], argv[3]);
  if (argc == 2 && strcmp(argv[1], "plan") == 0) return plan_mode();
  fprintf(stderr, "usage: %s run <in> <out> | %s plan\n", argv[0], argv[0]);
  return 2;
}
