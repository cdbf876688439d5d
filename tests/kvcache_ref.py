"""One fp64 definition of the KV-cache forward family — flash_attn_with_kvcache in its 4-D form, with cu_seqlens_q (packed query rows), scheduler_metadata,
fp8 caches, pack_gqa, num_splits, k= / v= and kvcache_append_varlen in front —, its per-element bounds, the cases tests/test_kvcache_fwd_bounds_gpu.py runs on
the GPU and tests/test_kvcache_bounds_cpu.py proves on the CPU, and the mutants the bounds must tell from the definition (tests only).

The definition (include/tfa.h), per sequence b with nq_b query rows and len_b keys: the keys are positions [0, len_b) of the cache, gathered through the block
table (key j is row j % page_size of page block_table[b, j / page_size]); an fp8 cache is decoded exactly and K / V multiplied by k_descale / v_descale[b, hk];
query head h reads K/V head hk = h // G; causal is bottom-right aligned, key j visible to row t iff j <= t + (len_b - nq_b); a row that sees no key gives
out = 0, lse = +inf.  The 4-D layout (q (B, Nq, H, D), nq_b = Nq) and the packed one (q (total_q, H, D), rows [q0_b, q0_b + nq_b) with the header's clamping)
are two views of this one function: both go through seq_problem / attend.  With k= / v= or kvcache_append_varlen in front the keys are what the append is
defined to leave in the cache (apply_append: row t of sequence b at position before_b + t; K rotated at that position when tables are given; an fp8 cache
stores rne_e4m3fn(clamp(x / descale, -448, 448)) of the 16-bit row, a true fp32 division).

Bounds, element by element:
  out (B2 form)   |out16 - ref| <= eps16 * A + 1e-6 + half an ulp16 of the result * (1 + 1e-3),   A = v_descale * sum_j P_ij |dec v_jd|
                  — include/tfa.h's "every path, fp32 output" guarantee plus the ONE rounding of O; splits do not change it (the partials and tfa_merge are
                  fp32, O is rounded once).  form_ref.ratios(half_ulp=True) is the arithmetic.
  lse             lse_bound below: a closed form in u = 2^-24, derived from the kernels' statements, nothing fitted.
"""
import math
import random

import torch

import form_ref as F
import rotary_ref as R

BF16, FP16, E4M3 = torch.bfloat16, torch.float16, torch.float8_e4m3fn
U = 2.0 ** -24
LN2 = 0.6931471805599453
LOG2E = 1.4426950408889634
ALPHA = 3.0                     # every q row's component along the hot direction (see build)
LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 300, 700)      # ... and the capacity
PACKED_LQ = [300, 1, 130, 0, 64]


def round_up(x, m):
    return (x + m - 1) // m * m


def chunk_of(n, splits):
    """include/tfa.h: chunk_b = round_up(ceil(len_b / splits), 64)."""
    return max(64, round_up((n + splits - 1) // splits, 64))


def lse_splits(c):
    """The number of parts tfa_merge can see: the case's num_splits; with num_splits = 0 (the library's choice, unknown here) the most chunks of at least
    one 64-key tile the capacity can be cut into."""
    return c["splits"] if c["splits"] else max(1, c["cap"] // 64)


def lse_bound(T, n, lse, D, splits):
    """|lse_kernel - lse_exact| <= u * [(D + 15) * T + 4 * ceil(n / 64) + 13] + 2^-22 * |lse|      (one chunk)
                                    ... + u * (5 * splits + 4) + u * |lse|                             (merged, splits > 1)
    T = max over the visible keys j of sc * sum_d |q_d| |k_jd| (sc = softmax_scale * k_descale, k decoded): the size of a score when nothing cancels.
    Every term is a statement of tfa_fwd_kernel_dma_body.inc (the one body of the family) or tfa_merge.hip; relative errors of the positive sum l become
    absolute errors of log l:
      D * T        sacc: the score's D products (exact in fp32: 16-bit x 16-bit) accumulated in fp32 by the MFMAs, at most one rounding per product (the
                   hardware rounds once per MFMA, D / 16 times); the score enters the exponent, so its absolute error is the LSE's.
      2 * T        sc = p.scale_log2 * kd: the host's rounding of scale * log2(e) and the product with k_descale move every exponent by 2u relative.
      2 * T        e = fast_exp2(fmaf(sacc, sc, -msc)): the fma's one rounding, |argument| <= (|s_j| + |m|) * sc <= 2 T / ln 2.
      1 * T        msc = m_new * sc: rounded once, and NOT the product the LSE uses (next line): the two do not cancel.
      3 * T        lse = m_run * scale_lse + ...: scale_lse = p.scale * kd (two roundings) and the product with m.
      4 * T        alpha = fast_exp2((m_run - m_new) * sc): the difference and the product are rounded (2u of the argument); the arguments of all rescalings
                   of a row telescope to (first maximum - last maximum) * sc <= 2 T / ln 2.
      3 * T        __builtin_amdgcn_logf(l_tot) * 0.693...: one ulp of v_log_f32 and the product, 3u * ln l, and ln l = lse - m * scale <= |lse| + T: the
                   |lse| part is in the last term.
      4 / tile     l_run *= alpha (one rounding, and fast_exp2's one ulp = 2u in alpha), l_run += (...) (one addition), per 64-key tile.
      13           fast_exp2 of every term (one ulp of v_exp_f32 = 2u); the in-tile partials lsum[r & 3] += e (8 terms each), (lsum[0] + lsum[1]) +
                   (lsum[2] + lsum[3]) and the addition into l_run: a term passes at most 10 additions; pair_sum(l_run) across the two half-waves: 1.
      2^-22 |lse|  3u |lse| from the log term above and the final addition m * scale + log l.
    Terms flushed to zero by v_exp_f32 are below 2^-126 of the row's largest and are not counted.
    Merged (tfa_merge.hip): every part's LSE carries the bound above, weighted by w_p / wsum; a part's own |lse_p| exceeds |lse| by d = lse - lse_p at
    weight e^-d, and d e^-d <= 1 / e: inside the 4.  Per part: l - m (u |l - m|, at weight e^-|l - m|: <= u), __expf = exp2(x * log2 e) (the product: <= u
    at that weight; exp2: 2u), wsum += w (u): 5 per part.  m + __logf(wsum): 3u ln(wsum) <= 3u ln(splits) (inside 5 * splits + 4) and the addition, u |lse|."""
    tiles = (n + 63) // 64
    b = U * ((D + 15) * T + 4 * tiles + 13) + 4 * U * lse.abs()
    if splits > 1:
        b = b + U * (5 * splits + 4) + U * lse.abs()
    return b


# ---- the definition -----------------------------------------------------------------------------------------------------------------------------
def gather(cache, bt, b, n, last_from=None):
    """Keys [0, n) of sequence b: (n, Hk, D) fp64, an fp8 cache decoded exactly.  last_from: the block-table row the LAST page is taken from (a mutant)."""
    if bt is None:
        x = cache[b, :n]
    else:
        page = cache.shape[1]
        npg = (n + page - 1) // page
        rows = [b] * npg
        if last_from is not None and npg:
            rows[-1] = last_from
        pages = [cache[int(bt[r, i])] for i, r in enumerate(rows)]
        x = torch.cat(pages, 0)[:n] if pages else cache[0, :0]
    return x.float().double()


MUTANTS = ("len-1", "len+1", "shift+1", "shift-1", "seam", "page_next", "v_tile", "kv_head_mod", "pack_pos", "descale_next", "kd_not_in_lse", "vd_twice",
           "len_next", "nq_unclamped", "new_unquantised")


def seq_problem(t, b, mut=None):
    """Sequence b as attend() takes it: dict(q (H, nq, D), k / v (H, n, D) decoded and NOT descaled, sck (H,) = softmax_scale * k_descale, vd (H,), vis
    (H, nq, n) bool, n, nq).  mut: what a wrong kernel would have read instead (MUTANTS) — the fp64 result of a wrong definition, not a change to a kernel."""
    c = t["case"]
    B, H, Hk, D, cap = t["B"], c["H"], c["Hk"], c["D"], c["cap"]
    G = H // Hk
    q0, nq = t["rows"][b]
    n = t["lens"][(b + 1) % B if mut == "len_next" else b]
    if mut == "len-1":
        n = max(n - 1, 0)
    elif mut == "len+1":
        n = min(n + 1, cap)
    bt = t["bt"]
    k = gather(t["k_final"], bt, b, n, (b + 1) % B if mut == "page_next" else None)
    v = gather(t["v_final"], bt, b, n, (b + 1) % B if mut == "page_next" else None)
    if mut == "v_tile" and n >= 128:                       # V of the first 64-key tile read one tile further, K right
        v[0:64] = v[64:128].clone()
    kd, vd = t["kd"][b].double(), t["vd"][b].double()      # (Hk,)
    if mut == "descale_next":
        kd, vd = kd.roll(-1), vd.roll(-1)
    if mut == "new_unquantised" and t["new"] is not None:   # the appended rows attended at 16-bit precision
        lo, xk, xv = t["new"][b]
        hi = min(lo + xk.shape[0], n)
        if hi > lo:
            k[lo:hi] = xk[:hi - lo].double() / kd.view(1, Hk, 1)
            v[lo:hi] = xv[:hi - lo].double() / vd.view(1, Hk, 1)
    hk_of = torch.arange(H) % Hk if mut == "kv_head_mod" else torch.arange(H) // G
    q = t["q"][q0:q0 + nq].double().transpose(0, 1)        # (H, nq, D)
    j = torch.arange(n).view(1, 1, n)
    vis = torch.ones(H, nq, n, dtype=torch.bool)
    if c["causal"]:
        pos = torch.arange(nq).view(1, nq).expand(H, nq)
        if mut == "pack_pos":                              # packed rows are position-major, row = t * G + g: the position taken as row % Nq
            row = torch.arange(nq).view(1, nq) * G + (torch.arange(H) % G).view(H, 1)
            pos = row % max(nq, 1)
        shift = n - (t["asked"][b] if mut == "nq_unclamped" else nq) + {"shift+1": 1, "shift-1": -1}.get(mut, 0)
        vis = vis & (j <= pos.unsqueeze(-1) + shift)
    if mut == "seam" and c["splits"] > 1:                  # the last key of every chunk that has a chunk behind it
        ch = chunk_of(n, c["splits"])
        for s in range(ch, n, ch):
            vis[:, :, s - 1] = False
    return dict(q=q, k=k[:, hk_of].transpose(0, 1), v=v[:, hk_of].transpose(0, 1), sck=t["sc"] * kd[hk_of], vd=vd[hk_of], vis=vis, n=n, nq=nq, mut=mut)


def scores(p):
    s = torch.einsum("hqd,hkd->hqk", p["q"], p["k"]) * p["sck"].view(-1, 1, 1)
    return s.masked_fill(~p["vis"], -math.inf)


def attend(p):
    """The definition on one seq_problem: out (nq, H, D), lse (H, nq) (+inf on a row that sees no key), A (nq, H, D), T (H, nq) (lse_bound's)."""
    H, nq, D = p["q"].shape
    if p["n"] == 0 or nq == 0:
        return (torch.zeros(nq, H, D, dtype=torch.float64), torch.full((H, nq), math.inf, dtype=torch.float64), torch.zeros(nq, H, D, dtype=torch.float64),
                torch.zeros(H, nq, dtype=torch.float64))
    s = scores(p)
    m = s.max(dim=-1, keepdim=True).values
    seen = torch.isfinite(m)
    e = torch.exp(s - torch.where(seen, m, torch.zeros_like(m)))
    l = e.sum(-1, keepdim=True)
    P = torch.where(seen, e / torch.where(seen, l, torch.ones_like(l)), torch.zeros_like(e))
    lse = torch.where(seen, m + torch.log(torch.where(seen, l, torch.ones_like(l))), torch.full_like(m, math.inf)).squeeze(-1)
    vd = p["vd"].view(-1, 1, 1)
    out, A = (P @ p["v"]) * vd, (P @ p["v"].abs()) * vd
    T = (torch.einsum("hqd,hkd->hqk", p["q"].abs(), p["k"].abs()) * p["sck"].view(-1, 1, 1)).masked_fill(~p["vis"], 0.0).max(dim=-1).values
    return out.transpose(0, 1), lse, A.transpose(0, 1), T


def attend_mut(t, b, mut):
    """The fp64 (out, lse) a kernel with defect `mut` would give for sequence b."""
    p = seq_problem(t, b, mut)
    out, lse, _, _ = attend(p)
    if mut == "kd_not_in_lse" and p["n"] and p["nq"]:      # lse = m_raw * softmax_scale + log l instead of m_raw * softmax_scale * k_descale + log l
        m = scores(p).max(dim=-1).values                   # (H, nq), = m_raw * softmax_scale * kd
        kd = (p["sck"] / t["sc"]).view(-1, 1)
        lse = torch.where(torch.isfinite(m), lse - m + m / kd, lse)
    if mut == "vd_twice":                                  # v_descale on the partials and again behind the merge
        out = out * p["vd"].view(1, -1, 1)
    return out, lse


def round16(x, dtype):
    return x.float().to(dtype).double()


def _chunks(n, splits):
    if splits <= 1:
        return [(0, n)]
    ch = chunk_of(n, splits)
    return [(s * ch, min(n, (s + 1) * ch)) for s in range(splits)]


def emulate16(t, b, dtype=None):
    """The kernels' algorithm on sequence b with their rounding points, fp64 elsewhere: per chunk (round_up(ceil(len_b / splits), 64) keys) the 64-key tile
    loop — P rounded to the 16-bit type against the exact running maximum, l summed from the unrounded P —, v_descale on every partial in front of the
    merge, the merge by the parts' LSEs, ONE rounding of O.  Returns out16 (nq, H, D) as fp64."""
    dtype = dtype or t["dtype"]
    p = seq_problem(t, b)
    H, nq, D = p["q"].shape
    if p["n"] == 0 or nq == 0:
        return torch.zeros(nq, H, D, dtype=torch.float64)
    s = scores(p)
    parts = []
    for lo, hi in _chunks(p["n"], t["case"]["splits"]):
        m = torch.full((H, nq, 1), -math.inf, dtype=torch.float64)
        l = torch.zeros(H, nq, 1, dtype=torch.float64)
        o = torch.zeros(H, nq, D, dtype=torch.float64)
        for t0 in range(lo, hi, 64):
            st = s[:, :, t0:min(t0 + 64, hi)]
            mn = torch.maximum(m, st.max(dim=-1, keepdim=True).values)
            safe = torch.where(torch.isfinite(mn), mn, torch.zeros_like(mn))
            alpha = torch.exp(m - safe)
            e = torch.exp(st - safe)
            l = l * alpha + e.sum(-1, keepdim=True)
            o = o * alpha + round16(e, dtype) @ p["v"][:, t0:min(t0 + 64, hi)]
            m = mn
        has = l > 0
        ls = torch.where(has, l, torch.ones_like(l))
        parts.append((torch.where(has, o / ls, torch.zeros_like(o)) * p["vd"].view(-1, 1, 1), torch.where(has, m + torch.log(ls), torch.full_like(m, -math.inf))))
    lses = torch.stack([x[1] for x in parts])              # (parts, H, nq, 1), -inf = an empty part
    M = lses.max(dim=0).values
    safe = torch.where(torch.isfinite(M), M, torch.zeros_like(M))
    w = torch.exp(lses - safe)
    ws = w.sum(0)
    o = (w * torch.stack([x[0] for x in parts])).sum(0) / torch.where(ws > 0, ws, torch.ones_like(ws))
    return round16(o, dtype).transpose(0, 1)


def emulate_lse32(t, b):
    """The LSE in the kernels' order and in fp32 throughout: fp32 scores, sc = fp32(scale * log2 e) * kd, exp2(fma(s, sc, -m * sc)), l summed tile by tile with
    the rescaling by exp2((m_old - m_new) * sc), lse = m * (scale * kd) + log2(l) * ln 2, and tfa_merge's m + log(sum exp(l_p - m)) over the parts.  (H, nq)."""
    p = seq_problem(t, b)
    H, nq, D = p["q"].shape
    f = torch.float32
    if p["n"] == 0 or nq == 0:
        return torch.full((H, nq), math.inf, dtype=f)
    kd = (p["sck"] / t["sc"]).to(f).view(-1, 1, 1)
    sc = torch.tensor(t["sc"] * LOG2E, dtype=f) * kd
    sl = torch.tensor(t["sc"], dtype=f) * kd
    raw = torch.einsum("hqd,hkd->hqk", p["q"].to(f), p["k"].to(f)).masked_fill(~p["vis"], -math.inf)
    parts = []
    for lo, hi in _chunks(p["n"], t["case"]["splits"]):
        m = torch.full((H, nq, 1), -1e30, dtype=f)
        l = torch.zeros(H, nq, 1, dtype=f)
        for t0 in range(lo, hi, 64):
            st = raw[:, :, t0:min(t0 + 64, hi)]
            mn = torch.maximum(m, st.max(dim=-1, keepdim=True).values)
            l = l * torch.exp2((m - mn) * sc)
            e = torch.exp2(st * sc - mn * sc)
            for i in range(e.shape[-1]):
                l = l + e[:, :, i:i + 1]
            m = mn
        parts.append(torch.where(l > 0, m * sl + torch.log2(torch.where(l > 0, l, torch.ones_like(l))) * torch.tensor(LN2, dtype=f), torch.full_like(l, math.inf)))
    if len(parts) == 1:
        return parts[0].squeeze(-1)
    ls = torch.stack(parts)
    fin = torch.isfinite(ls)
    M = torch.where(fin, ls, torch.full_like(ls, -math.inf)).max(dim=0).values
    w = torch.where(fin, torch.exp(ls - torch.where(torch.isfinite(M), M, torch.zeros_like(M))), torch.zeros_like(ls)).sum(0)
    return torch.where(w > 0, M + torch.log(torch.where(w > 0, w, torch.ones_like(w))), torch.full_like(w, math.inf)).squeeze(-1)


# ---- the ratios -----------------------------------------------------------------------------------------------------------------------------------
def out_ratio(out, ref, A, dtype):
    """max(|out - ref| / bound) with the (B2) bound of form_ref.ratios; a NaN counts as infinitely far out."""
    if out.numel() == 0:
        return 0.0
    if bool(torch.isnan(out).any()):
        return math.inf
    return F.ratios([out], [ref], [A], dtype, half_ulp=True)[0]


def lse_ratio(lse, ref, T, n, D, splits):
    """max(|lse - ref| / lse_bound) over the rows that see a key; +inf on other rows than the reference, or a NaN, counts as infinitely far out."""
    lse, ref = lse.double(), ref.double()
    if lse.numel() == 0:
        return 0.0
    fin = torch.isfinite(ref)
    if bool(torch.isnan(lse).any()) or not torch.equal(torch.isposinf(lse), torch.isposinf(ref)):
        return math.inf
    if not bool(fin.any()):
        return 0.0
    return ((lse[fin] - ref[fin]).abs() / lse_bound(T[fin], n, ref[fin], D, splits)).max().item()


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------
def _case(id, **kw):
    """form: "4d" (Nq) or "packed" (lq, max_q); page 0 = a contiguous cache; splits 0 = the library's choice; pack: pack_gqa; sched: through scheduler_metadata;
    append: None, "4d" (k= / v=, n_new rows) or "varlen" (kvcache_append_varlen with q= and rotary tables in front, the new rows are the query rows')."""
    c = dict(id=id, form="4d", dtype=BF16, B=None, H=4, Hk=4, D=64, Nq=1, lq=None, max_q=None, lens=None, cap=512, page=0, causal=False, splits=1, fp8=False,
             pack=None, sched=False, append=None, n_new=0, long=False, auto=False, seed=0)
    c.update(kw)
    c["B"] = len(c["lens"])
    if c["form"] == "packed":
        assert len(c["lq"]) == c["B"]
        c["max_q"] = c["max_q"] or max(1, max(c["lq"]))
    c["mutants"], c["na"] = name_mutants(c)
    return c


def rows_of(c):
    """(q0_b, nq_b) as the header clamps them, and the row counts asked for."""
    if c["form"] == "4d":
        return [(b * c["Nq"], c["Nq"]) for b in range(c["B"])], [c["Nq"]] * c["B"]
    total, rows, q0 = sum(c["lq"]), [], 0
    for n in c["lq"]:
        rows.append((q0, min(n, c["max_q"], total - q0)))
        q0 += n
    return rows, list(c["lq"])


def packs(c):
    """Whether the call runs GQA heads as packed position-major rows (ops.flash_attn_with_kvcache's docstring)."""
    G = c["H"] // c["Hk"]
    if G == 1 or c["pack"] is False:
        return False
    return True if c["form"] == "packed" else (c["pack"] is True or c["Nq"] == 1)


def name_mutants(c):
    """(the mutants a case can have, [(mutant, why not)] for the others) — structural: which defect has something to act on in this case."""
    rows, asked = rows_of(c)
    G = c["H"] // c["Hk"]
    live = [(n, nq, a) for n, (_, nq), a in zip(c["lens"], rows, asked) if nq > 0]
    ok, na = [], []

    def put(m, cond, why):
        ok.append(m) if cond else na.append((m, why))

    put("len-1", any(n >= 1 for n, _, _ in live), "no sequence with a key and a row")
    put("len+1", not c["fp8"] and any(n < c["cap"] for n, _, _ in live), "fp8: the tail holds NaN codes, the NaN assertion's business" if c["fp8"] else "every length is the capacity")
    put("shift+1", c["causal"] and any(nq >= 2 and n >= 1 for n, nq, _ in live), "no causal diagonal below the last row")
    put("shift-1", c["causal"] and any(n >= 1 for n, _, _ in live), "not causal")
    put("seam", c["splits"] > 1 and any(n > chunk_of(n, c["splits"]) for n, _, _ in live), "one chunk per sequence (or the library's own split count)")
    put("page_next", c["page"] > 0 and c["B"] > 1 and any(n >= 1 for n, _, _ in live), "a contiguous cache" if not c["page"] else "one sequence")
    put("v_tile", any(n >= 128 for n, _, _ in live), "no sequence with two whole tiles")
    put("kv_head_mod", G > 1 and c["Hk"] > 1, "G = 1: h % Hk == h // G" if G == 1 else "MQA: one K/V head")
    put("pack_pos", packs(c) and c["causal"] and any(nq >= 2 and n >= 1 for n, nq, _ in live), "rows not packed, not causal, or one position")
    put("descale_next", c["fp8"] and c["Hk"] > 1, "MQA: one descale per sequence" if c["fp8"] else "no fp8 cache")
    put("kd_not_in_lse", c["fp8"], "no fp8 cache")
    put("vd_twice", c["fp8"] and c["splits"] > 1, "no merge behind the partials" if c["fp8"] else "no fp8 cache")
    put("len_next", c["form"] == "packed" and c["B"] > 1 and len(set(c["lens"])) > 1, "4-D: the launch indexes the batch by its grid")
    put("nq_unclamped", c["form"] == "packed" and c["causal"] and any(a > nq and n >= 1 for n, nq, a in live), "no nq_b above max_seqlen_q (or not causal)")
    put("new_unquantised", c["fp8"] and c["append"] is not None, "no fp8 append")
    return ok, na


def _packed(id, **kw):
    return _case(id, form="packed", lq=PACKED_LQ, **kw)


def _cases():
    cs = [
        # 4-D, 16-bit caches
        _case("4d-bf16-d40-g1-nq1", dtype=BF16, D=40, H=4, Hk=4, Nq=1, lens=[700, 1, 63, 64, 1024], cap=1024, seed=1),
        _case("4d-fp16-d64-g2-nq5-causal-page64-s2", dtype=FP16, D=64, H=4, Hk=2, Nq=5, lens=[65, 127, 128, 1, 300], cap=512, page=64, causal=True, splits=2, seed=2),
        _case("4d-bf16-d104-g4-nq1-page128-s3", dtype=BF16, D=104, H=8, Hk=2, Nq=1, lens=[129, 700, 0, 1024], cap=1024, page=128, splits=3, seed=3),
        _case("4d-fp16-d128-mqa-nq5-causal-s4-pack", dtype=FP16, D=128, H=8, Hk=1, Nq=5, lens=[300, 64, 1], cap=512, causal=True, splits=4, pack=True, seed=4),
        _case("4d-bf16-d128-g4-nq130-causal-page256-unpacked", dtype=BF16, D=128, H=8, Hk=2, Nq=130, lens=[700, 129, 1024], cap=1024, page=256, causal=True,
              pack=False, seed=5),
        _case("4d-fp16-d64-g4-nq33-causal-s2-pack", dtype=FP16, D=64, H=8, Hk=2, Nq=33, lens=[300, 65, 512], cap=512, causal=True, splits=2, pack=True, seed=6),
        _case("4d-bf16-d64-g1-nq1-len65-s4", dtype=BF16, D=64, H=4, Hk=4, Nq=1, lens=[65, 128, 1], cap=256, splits=4, seed=7),          # 65 keys, 4 chunks: two empty
        _case("4d-bf16-d128-g4-nq1-page256-auto", dtype=BF16, D=128, H=8, Hk=2, Nq=1, lens=[700, 300, 129], cap=4096, page=256, splits=0, auto=True, seed=8),
        _case("4d-fp16-d40-g2-nq1-page64-unpacked", dtype=FP16, D=40, H=4, Hk=2, Nq=1, lens=[127, 256, 64], cap=256, page=64, pack=False, seed=9),
        _case("4d-bf16-d128-g4-nq1-5000-s8", dtype=BF16, D=128, H=8, Hk=2, Nq=1, lens=[5000], cap=5000, splits=8, long=True, seed=10),
        _case("4d-fp16-d64-g4-nq1-5000-s8", dtype=FP16, D=64, H=8, Hk=2, Nq=1, lens=[5000], cap=5000, splits=8, long=True, seed=11),
        # 4-D, fp8 caches
        _case("4d-fp8-bf16-d48-g2-nq1", dtype=BF16, D=48, H=4, Hk=2, Nq=1, lens=[300, 129], cap=512, fp8=True, seed=20),
        _case("4d-fp8-fp16-d64-g4-nq5-causal-page128-s3-pack", dtype=FP16, D=64, H=8, Hk=2, Nq=5, lens=[512, 65, 1], cap=512, page=128, causal=True, splits=3,
              pack=True, fp8=True, seed=21),
        _case("4d-fp8-bf16-d112-g1-nq1-page64-s2", dtype=BF16, D=112, H=4, Hk=4, Nq=1, lens=[127, 300], cap=512, page=64, splits=2, fp8=True, seed=22),
        _case("4d-fp8-fp16-d128-mqa-nq5-causal", dtype=FP16, D=128, H=8, Hk=1, Nq=5, lens=[64, 128, 0, 63], cap=256, causal=True, fp8=True, seed=23),
        # 4-D with k= / v=: append, then attend
        _case("4d-append-fp16-d104-g1-nq5-causal", dtype=FP16, D=104, H=4, Hk=4, Nq=5, lens=[300, 64, 128], cap=512, causal=True, append="4d", n_new=5, seed=30),
        _case("4d-append-fp8-bf16-d64-g2-nq3-causal-page64-s2", dtype=BF16, D=64, H=4, Hk=2, Nq=3, lens=[64, 129], cap=256, page=64, causal=True, splits=2,
              fp8=True, append="4d", n_new=3, seed=31),
        # packed q (cu_seqlens_q): a length shorter than its nq_b (128 < 300), the capacity, and 0
        _packed("vq-bf16-d64-g4-causal", dtype=BF16, D=64, H=8, Hk=2, lens=[128, 700, 1024, 65, 0], cap=1024, causal=True, seed=40),
        _packed("vq-fp16-d128-g2-causal-page128-s3-unpacked", dtype=FP16, D=128, H=4, Hk=2, lens=[128, 700, 1024, 65, 0], cap=1024, page=128, causal=True,
                splits=3, pack=False, seed=41),
        _packed("vq-bf16-d40-g1-page64-s2", dtype=BF16, D=40, H=4, Hk=4, lens=[128, 700, 1024, 65, 0], cap=1024, page=64, splits=2, seed=42),
        _packed("vq-fp8-fp16-d112-g2-causal-page256-pack", dtype=FP16, D=112, H=4, Hk=2, lens=[128, 700, 1024, 65, 0], cap=1024, page=256, causal=True, pack=True,
                fp8=True, seed=43),
        _packed("vq-bf16-d128-g2-causal-s2-maxq128", dtype=BF16, D=128, H=4, Hk=2, lens=[700, 300, 1024, 65, 0], cap=1024, causal=True, splits=2, max_q=128, seed=44),
        # kvcache_append_varlen (q= rotated in the launch) in front of the packed call
        _packed("vq-append-bf16-d64-g2-causal-page128-s2", dtype=BF16, D=64, H=4, Hk=2, lens=[300, 700, 1024, 65, 64], cap=1024, page=128, causal=True, splits=2,
                append="varlen", seed=50),
        _packed("vq-append-fp8-fp16-d48-g2-causal-page64", dtype=FP16, D=48, H=4, Hk=2, lens=[300, 700, 1024, 65, 64], cap=1024, page=64, causal=True, fp8=True,
                append="varlen", seed=51),
    ]
    by = {c["id"]: c for c in cs}
    for base in ("vq-bf16-d64-g4-causal", "vq-fp16-d128-g2-causal-page128-s3-unpacked", "vq-fp8-fp16-d112-g2-causal-page256-pack"):   # the scheduled form: the same result
        c = dict(by[base], id=base + "-sched", sched=True)
        cs.append(c)
    return cs


CASES = _cases()
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES), "case ids must be unique"


def sweep_case(seed):
    """test_seeded_sweep's draw, from the ranges of the list: dtype, fp8 or not, D of that kind, G in {1, 2, 4, 8} with H <= 8, B in 1..4, 4-D (Nq in
    {1, 5, 33, 130}) or packed rows, lengths from LENGTHS and the capacity, capacity in {256, 512, 1024}, contiguous or pages of 64 / 128 / 256, 1..4 splits,
    causal or not, pack_gqa None / True / False, the scheduled form on a third of the packed draws."""
    r = random.Random(7000 + seed)
    fp8 = r.random() < 0.3
    G = r.choice([1, 2, 4, 8])
    Hk = r.choice([h for h in (1, 2, 4) if h * G <= 8])
    B = r.randint(1, 4 if not fp8 else max(1, min(4, 10 // Hk)))
    cap = r.choice([256, 512, 1024])
    lens = [min(r.choice(LENGTHS + (cap,)), cap) for _ in range(B)]
    lens[0] = max(lens[0], 1)
    kw = dict(dtype=r.choice([BF16, FP16]), D=r.choice([48, 64, 112, 128] if fp8 else [40, 64, 104, 128]), H=G * Hk, Hk=Hk, lens=lens, cap=cap,
              page=r.choice([0, 64, 128, 256]), causal=r.random() < 0.5, splits=r.randint(1, 4), pack=r.choice([None, True, False]), fp8=fp8, seed=7000 + seed)
    if r.random() < 0.5:
        lq = [r.choice([0, 1, 1, 5, 33, 64, 130]) for _ in range(B)]
        lq[0] = max(lq[0], 1)
        return _case(f"sweep{seed}", form="packed", lq=lq, sched=r.random() < 0.34, **kw)
    return _case(f"sweep{seed}", Nq=r.choice([1, 1, 5, 33, 130]), **kw)


def case_of(case_id):
    return BY_ID[case_id] if case_id in BY_ID else sweep_case(int(case_id[len("sweep"):]))


# ---- the tensors of a case ------------------------------------------------------------------------------------------------------------------------------
def _randn(g, *shape, std=1.0):
    return torch.randn(*shape, generator=g, dtype=torch.float32) * std


def quantise(x16, d):
    """The append's fp8 byte: rne_e4m3fn(clamp(float(x) / descale, -448, 448)), a true fp32 division (x (..., Hk, D) 16-bit, d (Hk,) fp32)."""
    return (x16.float() / d.float().view(-1, 1)).clamp(-448.0, 448.0).to(E4M3)


def rot_tables(ro, D, dtype):
    """Rotary tables whose every angle is a multiple of 90 degrees, pos * (1 + i % 3) quarter turns at frequency i: cos and sin are 0 or +-1, so the rotation
    moves and negates elements and is exact in any arithmetic — a row rotated at another position than its key's gives another q."""
    quarter = (torch.arange(ro).view(ro, 1) * (1 + torch.arange(D // 2).view(1, D // 2) % 3)) % 4
    return torch.tensor([1.0, 0.0, -1.0, 0.0])[quarter].to(dtype), torch.tensor([0.0, 1.0, 0.0, -1.0])[quarter].to(dtype)


def hot_keys(c, n, tail=True):
    """The keys where an indexing error lives: the first, the last, the first behind the length, the first of the last page (or tile), the last of every chunk
    that has a chunk behind it."""
    if n == 0:
        return [0] if tail and c["cap"] > 0 else []
    unit = c["page"] or 64
    hot = {0, n - 1, (n - 1) // unit * unit}
    if tail and n < c["cap"]:
        hot.add(n)
    if c["splits"] > 1:
        ch = chunk_of(n, c["splits"])
        hot |= {s - 1 for s in range(ch, n, ch)}
    return sorted(hot)


def build(case, dtype=None):
    """The tensors of a case, on the CPU.  What the call gets: q_call, k_cache / v_cache (paged through bt when the case has pages; in the state BEFORE an
    append), lens_call (cache_seqlens as the attention call takes them), cu, kd / vd, and for an append k_new / v_new, before, cos / sin.  What the definition
    reads: q (rows, H, D) as attended, k_final / v_final (the caches behind the append, apply_append), lens, rows, asked, new.
    The inputs give the hot_keys weight: q std 1 and K / V std 0.5 as the family's other tests, plus a component ALPHA along one unit direction e in every q
    row and beta_b * e in sequence b's hot keys, beta_b such that the hot keys together hold about half of a row's probability (exp(bump) = 1.6 * cold keys /
    hot keys) — a single dropped, added or misplaced key then moves out and lse by percents, at any length.  Behind the lengths: finite garbage (std 1, the
    first key behind the length hot) in 16-bit caches, the NaN code in fp8 caches; spare pages: garbage of std 3 / NaN codes."""
    c = case
    dt = dtype or c["dtype"]
    B, H, Hk, D, cap = c["B"], c["H"], c["Hk"], c["D"], c["cap"]
    g = torch.Generator().manual_seed(1000 + c["seed"])
    sc = 1.0 / math.sqrt(D)
    rows, asked = rows_of(c)
    total = sum(c["lq"]) if c["form"] == "packed" else B * c["Nq"]
    e = (torch.randint(0, 2, (D,), generator=g).float() * 2 - 1) / math.sqrt(D)
    q = (_randn(g, total, H, D) + ALPHA * e).to(dt)
    lens = [min(max(n, 0), cap) for n in c["lens"]]
    xk, xv = _randn(g, B, cap, Hk, D, std=0.5), _randn(g, B, cap, Hk, D, std=0.5)
    for b, n in enumerate(lens):
        xk[b, n:] *= 2.0
        xv[b, n:] *= 2.0
        hot = hot_keys(c, n)
        bump = max(1.0, math.log(max(n - len(hot), 1) / max(len(hot), 1)) + 0.5)
        for j in hot:
            xk[b, j] += bump / (sc * ALPHA) * e
    xk, xv = xk.to(dt), xv.to(dt)
    t = dict(case=c, dtype=dt, sc=sc, B=B, rows=rows, asked=asked, lens=lens, q=q, q_call=q, total_q=total, new=None, cos=None, sin=None, k_new=None, v_new=None,
             cu=None, before=None)
    if c["fp8"]:
        idx = torch.randperm(B * Hk, generator=g).view(B, Hk).float()
        t["kd"], t["vd"] = 0.01 * 1.5 ** idx, 0.008 * 1.5 ** idx.flip(1).flip(0)        # pairwise at least 1.5x apart
        kc = torch.stack([quantise(xk[b], t["kd"][b]) for b in range(B)])
        vc = torch.stack([quantise(xv[b], t["vd"][b]) for b in range(B)])
        for b, n in enumerate(lens):
            kc.view(torch.uint8)[b, n:] = 0x7F
            vc.view(torch.uint8)[b, n:] = 0x7F
    else:
        t["kd"], t["vd"] = torch.ones(B, Hk), torch.ones(B, Hk)
        kc, vc = xk.clone(), xv.clone()
    raw = torch.uint8 if c["fp8"] else torch.int16
    if c["form"] == "packed":
        t["cu"] = F.cu_of(c["lq"])
    # an append: the rows [before_b, len_b) are what the append brings; the cache in front of it holds garbage there
    if c["append"] is not None:
        nnew = [c["n_new"]] * B if c["append"] == "4d" else list(c["lq"])
        before = [n - m for n, m in zip(lens, nnew)]
        assert min(before) >= 0
        t["before"] = torch.tensor(before, dtype=torch.int32)
        new_k = [xk[b, before[b]:lens[b]] for b in range(B)]
        new_v = [xv[b, before[b]:lens[b]] for b in range(B)]
        t["new"] = [(before[b], new_k[b], new_v[b]) for b in range(B)]
        for b in range(B):
            if c["fp8"]:
                kc.view(raw)[b, before[b]:lens[b]] = 0x7F
                vc.view(raw)[b, before[b]:lens[b]] = 0x7F
            else:
                kc[b, before[b]:lens[b]] = _randn(g, lens[b] - before[b], Hk, D, std=3.0).to(dt)
                vc[b, before[b]:lens[b]] = _randn(g, lens[b] - before[b], Hk, D, std=3.0).to(dt)
        if c["append"] == "4d":
            t["k_new"], t["v_new"] = torch.stack(new_k), torch.stack(new_v)
        else:                                              # packed rows, K and q handed over un-rotated: the launch rotates both at position before_b + t
            t["cos"], t["sin"] = rot_tables(cap, D, dt)
            pos, valid = R.packed_positions(total, [int(x) for x in t["cu"]], before)
            unrot = lambda x: R.rotary_ref64(x, t["cos"], t["sin"], pos, False, conjugate=True, valid=valid)[0].to(dt)   # noqa: E731
            t["k_new"], t["v_new"], t["q_call"] = unrot(torch.cat(new_k)), torch.cat(new_v), unrot(q)
            for x, want in ((t["k_new"], torch.cat(new_k)), (t["q_call"], q)):
                assert torch.equal(R.rotary_ref64(x, t["cos"], t["sin"], pos, False, valid=valid)[0], want.double()), "the quarter-turn rotation is exact"
    t["lens_call"] = torch.tensor(lens, dtype=torch.int32) if c["append"] != "4d" else t["before"]
    # pages: a shuffled table, three spare pages of garbage
    t["bt"] = None
    if c["page"]:
        page = c["page"]
        assert cap % page == 0
        mb = cap // page
        nb = B * mb + 3
        bt = torch.randperm(nb, generator=g)[:B * mb].view(B, mb).to(torch.int32)
        pools = []
        for x in (kc, vc):
            pool = torch.full((nb, page, Hk, D), 0x7F, dtype=torch.uint8).view(E4M3) if c["fp8"] else _randn(g, nb, page, Hk, D, std=3.0).to(dt)
            for b in range(B):
                for i in range(mb):
                    pool.view(raw)[int(bt[b, i])] = x.view(raw)[b, i * page:(i + 1) * page]
            pools.append(pool)
        kc, vc = pools
        t["bt"] = bt
    t["k_cache"], t["v_cache"] = kc, vc
    t["k_final"], t["v_final"] = apply_append(t) if c["append"] is not None else (kc, vc)
    return t


def apply_append(t):
    """What k= / v= and kvcache_append_varlen are defined to leave in the caches: row r of sequence b at key position before_b + r (dropped at or beyond the
    capacity), through the block table; K rotated at that position first when the case has tables (one 16-bit rounding; exact here); an fp8 cache takes
    quantise() of the 16-bit row with the sequence's descales."""
    c = t["case"]
    kc, vc = t["k_cache"].clone(), t["v_cache"].clone()
    raw = torch.uint8 if c["fp8"] else torch.int16
    r0 = 0
    for b in range(t["B"]):
        lo = int(t["before"][b])
        m = c["n_new"] if c["append"] == "4d" else c["lq"][b]
        if c["append"] == "4d":
            kn, vn = t["k_new"][b], t["v_new"][b]
        else:
            kn, vn = t["k_new"][r0:r0 + m], t["v_new"][r0:r0 + m]
            pos = torch.arange(lo, lo + m)
            kn = R.rotary_ref64(kn, t["cos"], t["sin"], pos, False)[0].float().to(t["dtype"])
        r0 += m
        if c["fp8"]:
            kn, vn = quantise(kn, t["kd"][b]), quantise(vn, t["vd"][b])
        for r in range(m):
            p = lo + r
            if not 0 <= p < c["cap"]:
                continue
            for cache, x in ((kc, kn), (vc, vn)):
                if t["bt"] is None:
                    cache.view(raw)[b, p] = x.view(raw)[r]
                else:
                    cache.view(raw)[int(t["bt"][b, p // c["page"]]), p % c["page"]] = x.view(raw)[r]
    return kc, vc


def reference(t):
    """Per sequence with rows: b -> (out (nq, H, D), lse (H, nq), A, T, n) in fp64."""
    return {b: attend(seq_problem(t, b)) + (t["lens"][b],) for b in range(t["B"]) if t["rows"][b][1] > 0}
