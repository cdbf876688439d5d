"""The prefill forward family — tfa_fwd by kernel variant, the local / ALiBi / softcap / bias forms, flash_attn_varlen_fwd, its paged form and
flash_attn_fwd_splitkv — held to per-element bounds on out and on the LSE: the bounds, the inputs, the cases tests/test_fwd_bounds_gpu.py runs on the GPU and
tests/test_fwd_bounds_cpu.py proves on the CPU, and the mutants the bounds must tell from the definition (tests only).

The definition is not restated here: form_ref.scores64 / ref_fwd / structure define every form in fp64 (score order: scale -> cap -> ALiBi -> bias -> mask),
kvcache_ref.gather defines paging, form_ref.sequences / seq_view the per-sequence views of a packed batch.  Added here: A = sum_j P_ij |v_jd| (ref_fwd returns
it), T (bound_terms), the bounds, and `attend`, the same function with one defect switched on (MUTANTS) — at "no defect" it is asserted equal to ref_fwd.

Bounds, element by element, no element exempt (include/tfa.h, "WHICH TOLERANCE EACH PATH GUARANTEES"):
  fp32 out     |d| <= eps16 * A + 1e-6
  16-bit out   |d| <= eps16 * A + 1e-6 + half an ulp16 of the result * (1 + 1e-3)       (form_ref.ratios(half_ulp=True); split-KV the same: partials and
               tfa_merge are fp32, O is rounded once)
  lse          lse_bound below: a closed form in u = 2^-24, derived from the kernels' statements, nothing fitted
  a row that sees no key: out = 0 and lse = +inf exactly.
"""
import math
import random

import torch

import form_ref as F
import kvcache_ref as K

BF16, FP16 = F.BF16, F.FP16
U = K.U
ALPHA = K.ALPHA                 # every q row's component along the hot direction (see build)
LOG2E = K.LOG2E


def tiles_of(n):
    return (n + 63) // 64


def lse_bound(T, n, lse, D, *, splits=1, slopes=False, bias=False, cap=0.0):
    """|lse_kernel - lse_exact| <= u * [(D + 15 + 2 [slopes] + 2 [bias]) * T + R * (T + ln n) + 11 * ceil(n / 64) + 3 ln n + 13 + 16 * cap] + 2^-22 * |lse|
                                    ... + u * (5 * splits + 4) + u * |lse|                                        (tfa_merge, splits > 1)
    T = max over the visible keys j of scale * sum_d |q_d| |k_jd| + slope * |i + shift - j| + |bias_ij|: the size of a score when nothing cancels (a capped
    score is smaller than its raw one, so T needs no cap); n = the keys of the sequence; R = 1 + floor(T / (20 ln 2)).  Three bodies compute an LSE of this
    family; the bound is the term-by-term maximum of theirs, because the dispatch (tfa_fwd_variant) is the library's business:

    (a) the issue-interleaved tile loop, tfa_fwd_kernel_il.h / tfa_fwd_il_tile_loop.inc / tfa_fwd_il_epilogue.inc (variants 30, 32, 36, 37, 38 and every
        form), and tfa_fwd_kernel_x4.h (variant 34), which carries the same statements (l4[rb][e & 3] += xs[n]; mref[rb] + __builtin_amdgcn_logf(l_tot)):
        the scores stay RAW (q.k), sc = scale * log2(e), lse = (mref + log2(l_tot)) * ln 2, relative errors of the positive sum l are absolute errors of log l.
      D * T        snext = mfma(kf, qf, snext): the score's D exact products accumulated in fp32, at most one rounding each; it enters the exponent.
      3 * T        sc = p.scale_log2 (the host's product scale * log2 e: two roundings) and the final "* 0.6931471805599453f" (the constant's rounding): the
                   kernel's log2 domain is (1 + 3u) off the natural one, d lse / d(that factor) = sum_j P_j x_j <= T.
      2 * T + ln n st_fma / soft_elem: xs = fmaf(s, sc, -msc), one rounding of an argument of size |s sc| + |mref|; |mref| ln 2 <= T under the lazy and the
                   exact rule (mref is an earlier row maximum) and <= T + ln n behind a 2^40 re-base (mref += e, 2^e <= l <= n * 2^(max - mref)).
      2 * T        rescale_if_needed / exact_step: alpha = fast_exp2(mref - nref): the difference is rounded, and the arguments of all re-bases of a row
                   telescope to (last reference - first) <= 2 T / ln 2.  (MAXFREE: alpha is an exact power of two; instead:)
      R * (T+ln n) MAXFREE's "mref += (float)e": the sum's rounding, u |mref + e|, moves everything summed so far by that factor; a row re-bases once per
                   2^40 of growth, and its sum cannot grow by more than 2 T / ln 2 bits: R = 1 + floor(2 T / (40 ln 2)) times.
      2 * (T+ln n) __builtin_amdgcn_logf(l_tot): one ulp of v_log_f32, 2u * ln l, l >= 1 under every rule (the row maximum's P is >= 1), and
                   ln l = lse - mref ln 2 <= |lse| + T + ln n; the |lse| part is in the last term.
      11 / tile    lsum[e & 3] += ev: the four partial sums run ACROSS the tiles, 8 additions each per tile (a lane holds 32 keys of a tile); l4[i] *= alpha:
                   one product, and fast_exp2's one ulp (2u) in alpha, per re-base, at most one per tile: 8 + 3.
      5            fast_exp2 of every term (one ulp = 2u); (l4[0] + l4[1]) + (l4[2] + l4[3]) (2 additions on a term's way) and pair_sum across the half-waves (1).
      6            KSPLIT (tfa_fwd_il_epilogue.inc): w = fast_exp2(mref - m) (the difference x at weight 2^-x: <= u; exp2: 2u), l_tot = w0 * l_tot + w1 * l1
                   (two products, one addition); each group's own partial carries the terms above over ITS tiles, fewer than ceil(n / 64).
      2^-22 |lse|  2u |lse| from the log term, the addition mref + log2 l and the product with ln 2: 4u |lse|.
      That is u * [(D + 9) * T + R * (T + ln n) + 11 * tiles + 3 ln n + 11] + 4u |lse|.
    (b) tfa_fwd_kernel_dma_body.inc (variant 17; the partial passes of tfa_fwd_splitkv at head dims up to 128): kvcache_ref.lse_bound, the same body:
        u * [(D + 15) * T + 4 * tiles + 13] + 4u |lse|.
    (c) tfa_merge.hip behind either: kvcache_ref.lse_bound's merged part, u * (5 * splits + 4) + u * |lse|.
    The forms add (tfa_fwd_kernel_il.h, apply_bias / bias_add), all on the raw scores in front of the mask and of everything above:
      2 * T        ALiBi: alibi_a = -slope / p.scale (the division's rounding, u * slope * distance) and s = fmaf(alibi_a, |cf - j|, s) (one rounding of the sum,
                   u * T); the distance itself is an exact small integer in fp32.
      2 * T        bias: bias_inv = 1.f / p.scale (one rounding) and s = fmaf(x, bias_inv, s) (one rounding); x itself is the bias element, 16-bit or fp32,
                   converted exactly.
      16 * cap     softcap: s = fmaf(-cap_cr, softcap_q(s, cap_k2), cap_cr) = cr * tanh(s / cr) with tanh within 2^-20 = 16u (include/tfa.h), cr = cap / scale:
                   an absolute 16u * cap in natural units.  tanh contracts, so the errors in front of it (D * T) pass it unenlarged."""
    tiles = tiles_of(n)
    ln_n = math.log(max(n, 2))
    R = 1 + torch.floor(T / (20 * math.log(2.0)))
    b = U * ((D + 15 + 2 * bool(slopes) + 2 * bool(bias)) * T + R * (T + ln_n) + 11 * tiles + 3 * ln_n + 13 + 16 * cap) + 4 * U * lse.abs()
    if splits > 1:
        b = b + U * (5 * splits + 4) + U * lse.abs()
    return b


def has_form(c):
    """Whether the case runs one of the forms' entry points (a true window, slopes, a cap or a bias) and not tfa_fwd / tfa_fwd_varlen themselves."""
    return c["slopes"] is not None or bool(c["cap"]) or c["bias"] is not None or F.eff_window(c["causal"], c["window"]) not in ((-1, -1), (-1, 0))


def old_lse_bar(lse, form):
    """What the suite asserted on an LSE before this file (include/tfa.h): 1e-4, and 1e-4 * max(1, |lse|) in the forms' tests."""
    return 1e-4 * lse.abs().clamp_min(1.0) if form else torch.full_like(lse, 1e-4)


def bound_terms(q, k, sc, **form):
    """T (B, H, Nq) of lse_bound for a (B,H,Nq,D) x (B,Hk,Nk,D) problem under `form` (form_ref.scores64's keywords)."""
    q64, k64 = F._f64(q), F._expand_kv(F._f64(k), q.shape[1])
    B, H, Nq, _ = q64.shape
    Nk = k64.shape[2]
    s, _ = F.scores64(q64, k64, sc, **form)
    t = sc * (q64.abs() @ k64.abs().transpose(-1, -2))
    if form.get("slopes") is not None:
        sl = F._f64(form["slopes"])
        sl = sl.view(1, H, 1, 1) if sl.dim() == 1 else sl.view(B, H, 1, 1)
        i, j = torch.arange(Nq, dtype=torch.float64).view(-1, 1), torch.arange(Nk, dtype=torch.float64).view(1, -1)
        t = t + sl.abs() * (i + (Nk - Nq) - j).abs()
    if form.get("bias") is not None:
        b = F._f64(form["bias"])
        t = t + torch.where(torch.isfinite(b), b.abs(), torch.zeros_like(b))
    return t.masked_fill(~torch.isfinite(s), 0.0).max(dim=-1).values


# ---- the definition with one defect switched on --------------------------------------------------------------------------------------------------
MUTANTS = ("wl+1", "wr+1", "shift+1", "shift-1", "alibi_shift0", "slopes_b0", "cap*1.02", "lse_uncapped", "lse_no_bias", "bias_row", "bias_kvhead", "next_key",
           "page_next", "v_tile", "kv_head_mod", "pack_pos", "seam", "len-1", "len+1")


def _mask(Nq, Nk, left, right, dshift=0, pos=None):
    i = (torch.arange(Nq) if pos is None else pos).view(-1, 1)
    j = torch.arange(Nk).view(1, -1)
    shift = Nk - Nq + dshift
    m = torch.ones(Nq, Nk, dtype=torch.bool)
    if left >= 0:
        m &= j >= i + shift - left
    if right >= 0:
        m &= j <= i + shift + right
    return m


def attend(part, sc, mut=None, splits=1):
    """(out, lse) in fp64 of one (1|B, H, n, D) problem — part = dict(q, k, v, form, and for the mutants that read beyond the keys k1 / v1 (one more row) or
    k_pn / v_pn (the keys with the LAST page taken from the next sequence's table row)) — as a kernel with defect `mut` would give it; None: the definition."""
    q, form = F._f64(part["q"]), dict(part["form"])
    k, v = part["k"], part["v"]
    extra = 0
    if mut in ("next_key", "len+1"):
        k, v, extra = part["k1"], part["v1"], 1
    elif mut == "page_next":
        k, v = part["k_pn"], part["v_pn"]
    k, v = F._f64(k), F._f64(v)
    B, H, Nq, D = q.shape
    Hk, Nk = k.shape[1], k.shape[2] - extra
    G = H // Hk
    hk = torch.arange(H) % Hk if mut == "kv_head_mod" else torch.arange(H) // G
    ke, ve = k[:, hk], v[:, hk]
    if mut == "v_tile" and Nk >= 128:                       # V of the first 64-key tile read one tile further, K right
        ve = ve.clone()
        ve[:, :, 0:64] = ve[:, :, 64:128]
    left, right = form.pop("window")
    dshift, pos, smut = 0, None, {}
    if mut == "wl+1":
        left += 1
    elif mut == "wr+1":
        right += 1
    elif mut in ("shift+1", "shift-1"):
        dshift = 1 if mut == "shift+1" else -1
    elif mut == "alibi_shift0":
        smut = {"alibi_shift0": True}
    elif mut == "slopes_b0":
        form["slopes"] = part["slopes_b0"]
    elif mut == "cap*1.02":
        form["softcap"] = form["softcap"] * 1.02
    elif mut == "bias_row":
        form["bias"] = torch.roll(form["bias"], 1, dims=2)
    elif mut == "bias_kvhead":
        form["bias"] = form["bias"][:, torch.arange(H) // G]
    elif mut == "pack_pos":                                 # packed GQA rows all at the last query position
        pos = torch.full((Nq,), Nq - 1)
    if extra:
        smut["extra_keys"] = 1

    def scores(f):
        s, _ = F.scores64(q, ke, sc, softcap=f.get("softcap", 0.0), slopes=f.get("slopes"), bias=f.get("bias"), window=(-1, -1), mut=smut)
        m = _mask(Nq, Nk, left, right, dshift, pos)
        if extra:
            m = torch.cat([m, torch.ones(Nq, 1, dtype=torch.bool)], dim=1)
        if mut == "len-1":
            m[:, Nk - 1] = False
        if mut == "seam" and splits > 1:                    # the last key of every chunk that has a chunk behind it
            ch = K.chunk_of(Nk, splits)
            for s0 in range(ch, Nk, ch):
                m[:, s0 - 1] = False
        return s.masked_fill(~m, -math.inf)

    def lse_of(s):
        empty = torch.isneginf(s).all(dim=-1)
        return torch.logsumexp(torch.where(empty.unsqueeze(-1), torch.zeros_like(s), s), dim=-1).masked_fill(empty, math.inf)

    s = scores(form)
    p, _ = F._probs(s)
    lse = lse_of(s)
    if mut == "lse_uncapped":
        lse = lse_of(scores(dict(form, softcap=0.0)))
    elif mut == "lse_no_bias":
        lse = lse_of(scores(dict(form, slopes=None, bias=None)))
    return p @ ve, lse


# ---- the ratios -----------------------------------------------------------------------------------------------------------------------------------
def out_ratio(out, ref, A, dtype, half_ulp):
    """max(|out - ref| / bound), the fp32 bound or (half_ulp) the 16-bit one; a NaN counts as infinitely far out."""
    if out.numel() == 0:
        return 0.0
    if bool(torch.isnan(out).any()):
        return math.inf
    return F.ratios([out], [ref], [A], dtype, half_ulp=half_ulp)[0]


def lse_ratio(lse, ref, bound):
    """max(|lse - ref| / bound) over the rows that see a key; +inf on other rows than the reference, or a NaN, counts as infinitely far out."""
    lse, ref = lse.double(), ref.double()
    if lse.numel() == 0:
        return 0.0
    fin = torch.isfinite(ref)
    if bool(torch.isnan(lse).any()) or not torch.equal(torch.isposinf(lse), torch.isposinf(ref)):
        return math.inf
    if not bool(fin.any()):
        return 0.0
    return ((lse[fin] - ref[fin]).abs() / bound[fin]).max().item()


def old_out_ratio(out, ref):
    """max |d| / 1e-2: the bar the suite held a 16-bit out to."""
    return ((out.double() - ref).abs().max().item() / 1e-2) if out.numel() else 0.0


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------
PAGES = (64, 256)               # tests/test_varlen_paged_gpu.py's
PLAIN_SHAPES = F.SHAPES + [(1, 300), (33, 65)]


def _case(id, **kw):
    """form_ref._case plus: kind "fixed" | "varlen" | "paged" | "splitkv" | "sliced"; layout; variant (-1: automatic dispatch); page; splits; peak (nats of
    the dominant key per batch entry, or None); Dfull / off (sliced: the width of the tensors the problem is a column slice of, and its first column)."""
    c = F._case(id, layout="bhnd", variant=-1, page=0, splits=1, peak=None, Dfull=0, off=0, hot=True)
    c.update(kw)
    c["mutants"], c["na"] = name_mutants(c)
    return c


def packed(c):
    return c["kind"] in ("varlen", "paged")


def shapes_of(c):
    """[(Nq, Nk)] of the case's parts: itself, or its sequences."""
    return list(zip(c["lq"], c["lk"])) if packed(c) else [(c["Nq"], c["Nk"])]


def packs_gqa(c):
    """Whether tfa_fwd runs the query heads of a K/V head as rows of one problem (tfa_api.hip: pack_gqa_rows) — automatic dispatch only."""
    if c["kind"] != "fixed" or c["variant"] >= 0 or c["H"] == c["Hk"] or c["layout"] != "bhnd" or c["slopes"] or c["cap"] or c["bias"] is not None:
        return False
    if F.eff_window(c["causal"], c["window"]) not in ((-1, -1), (-1, 0)):
        return False
    G = c["H"] // c["Hk"]
    return G * c["Nq"] <= 128 and (c["Nq"] == 1 or not c["causal"] or (c["D"] <= 128 and c["Nk"] >= c["Nq"]))


def name_mutants(c):
    """(the mutants a case can have, [(mutant, why not)] for the others) — structural: which defect has something to act on in this case."""
    left, right = F.eff_window(c["causal"], c["window"])
    live = [(nq, nk) for nq, nk in shapes_of(c) if nq > 0 and nk > 0]
    G = c["H"] // c["Hk"]
    B = len(c["lq"]) if packed(c) else c["B"]
    ok, na = [], []

    def put(m, cond, why):
        ok.append(m) if cond else na.append((m, why))

    put("wl+1", any(0 <= left < nk - 1 for _, nk in live), "left edge unbounded or beyond the first key")
    put("wr+1", any(0 <= right < nq - 1 for nq, _ in live), "right edge unbounded or beyond the last key")
    put("shift+1", right == 0 and any(nq >= 2 for nq, _ in live), "no causal diagonal below the last row")
    put("shift-1", right == 0, "no causal diagonal")
    shift0 = c["slopes"] is not None and any(F._shift0_applies(c["causal"], c["window"], nq, nk)[0] for nq, nk in live)
    put("alibi_shift0", shift0, "no slopes" if c["slopes"] is None else "Nq == Nk, or a right edge of 0 with Nq > Nk: the distances move by a row constant")
    put("slopes_b0", c["slopes"] == "BH" and B > 1, "one slope row for the batch")
    near = c["cap"] >= 50
    put("cap*1.02", bool(c["cap"]) and not near, "near linear: |x / cap| < 0.03, the cap moves nothing above eps16" if near else "no cap")
    put("lse_uncapped", bool(c["cap"]) and not near, "near linear: the capped and the raw scores agree to 1e-3 relative" if near else "no cap")
    put("lse_no_bias", c["slopes"] is not None or c["bias"] is not None, "no ALiBi and no bias term")
    put("bias_row", c["bias"] is not None, "no bias")
    put("bias_kvhead", c["bias"] is not None and c["bias"]["shape"][1] and c["bias"]["layout"] != "expanded" and 1 < c["Hk"] < c["H"],
        "no bias" if c["bias"] is None else "G = 1, MQA, or one bias slice for every head")
    put("next_key", c["kind"] == "varlen", "no second sequence in the tensor" if not packed(c) else "paged: the row behind the length is the page's own (len+1)")
    put("page_next", c["kind"] == "paged" and B > 1, "no page table" if c["kind"] != "paged" else "one sequence")
    first_tile_seen = any(nk >= 128 and (left < 0 or nk - nq - left < 64) for nq, nk in live)          # (row 0 reaches furthest left)
    put("v_tile", first_tile_seen and not (c["peak"] is not None and not c["causal"]),
        "the dominant key holds all but e^-20 of every row" if c["peak"] is not None else "no sequence with two whole tiles whose first tile a row sees")
    put("kv_head_mod", G > 1 and c["Hk"] > 1, "G = 1: h % Hk == h // G" if G == 1 else "MQA: one K/V head")
    put("pack_pos", packs_gqa(c) and c["causal"] and c["Nq"] >= 2, "rows not packed (forced variant, a form, G = 1 or G * Nq > 128), not causal, or one position")
    put("seam", c["kind"] == "splitkv" and any(nk > K.chunk_of(nk, c["splits"]) for _, nk in live), "one chunk")
    tail_masked = c["bias"] is not None and c["bias"]["masked"] and any(nk > 64 for _, nk in live)
    flat = bool(c["cap"]) and c["std"] >= 8 and c["dtype"] == BF16
    put("len-1", bool(live) and c["peak"] is None and not tail_masked and not flat,
        "the dominant key holds all but e^-20 of the rows that see the last key" if c["peak"] is not None else
        "the bias masks the last key tile for every row" if tail_masked else
        "saturated cap in bf16: the cap flattens the hot keys, every visible key holds about 1 / n of a row, within 10x of eps16" if flat else
        "no sequence with a key and a row")
    put("len+1", c["kind"] == "paged", "the row behind the last key is no row of the tensor (packed: next_key)" if c["kind"] != "varlen" else "packed: next_key is this defect")
    return ok, na


def il_instantiation(variant, Nq, D):
    """tfa_launch.h: il_instantiation for a (b,h) slice below 2 GiB and unpacked rows — which instantiation of a forced il variant a problem runs: "idle" (a
    single partial query block: Nq <= block rows - 32), "narrow" (il8 / il4 at a head dim that leaves the kernel's last 32 columns empty) or "main", the one with
    the hand-scheduled statement and, for bf16, TFA_RULE_FIRST_TILE.  None for the kernels without such forms (17, 34)."""
    if variant == 38:
        return "main"
    if variant not in (30, 32, 36, 37):
        return None
    if Nq <= (256 if variant == 30 else 128) - 32:
        return "idle"
    if variant in (30, 32) and D <= (64 if D <= 64 else 128) - 32:
        return "narrow"
    return "main"


BIG_SHAPES = [(257, 130), (320, 385)]        # more than 224 rows: past the idle-wave instantiation of the 256-row kernel (variant 30), and of the 128-row ones
SMALL_SHAPES = [s for s in PLAIN_SHAPES if s not in BIG_SHAPES]


def _plain_cases():
    """Every product variant that serves the width, forced, plus automatic dispatch, three times each: in both dtypes on the two shapes that reach the variant's
    product instantiation (main; narrow for il8 / il4 at D 96 — a block of at most 224 / 96 rows runs the idle-wave instantiation instead, another
    epilogue), causal on one and not on the other, and once on a smaller shape; H / Hk, batch and layout rotate (form_ref._cases' scheme)."""
    cs = []
    dts, hks = [BF16, FP16], [4, 2, 1]
    serve = {128: [-1, 30, 32, 36, 37, 38, 17], 64: [-1, 30, 32, 36, 37, 38, 17], 40: [-1] + NARROW_VARIANTS, 96: [-1] + NARROW_VARIANTS, 136: [-1], 256: [-1]}
    n = 0
    for D, variants in serve.items():
        for vi, var in enumerate(variants):
            for rep in range(3):
                Nq, Nk = BIG_SHAPES[(n + rep) % 2] if rep < 2 else SMALL_SHAPES[n % len(SMALL_SHAPES)]
                causal = bool(rep & 1) ^ bool(vi & 1)
                cs.append(_case(f"plain-d{D}-v{var if var >= 0 else 'auto'}-{'c' if causal else 'f'}-{Nq}x{Nk}", D=D, variant=var, dtype=dts[(n + rep) % 2],
                                Hk=hks[(n + rep) % 3], B=1 + (n % 2), Nq=Nq, Nk=Nk, causal=causal, layout=("bhnd", "bnhd")[(n // 2 + rep) % 2], seed=2000 + 3 * n + rep))
            n += 1
    for i, dt in enumerate(dts):                             # the GQA row packing of pack_gqa_rows: row % Nq carries the query position
        cs.append(_case(f"plain-pack-{'bf16' if dt == BF16 else 'fp16'}-4x200", D=128 >> i, H=8, Hk=2, dtype=dt, Nq=4, Nk=200, causal=True, seed=2200 + i))
    cs.append(_case("plain-pack-fp16-33x65", D=64, H=4, Hk=2, dtype=FP16, Nq=33, Nk=65, causal=True, seed=2202))
    return cs


NARROW_VARIANTS = [30, 32, 36, 37, 38, 17]  # tfa_launch.h: supports_padded_d — every product variant up to 128 wide serves the head dims below its width


def _form_cases():
    """form_ref.CASES' form parameters (the nine windows, the ALiBi, softcap and bias rows, the six packed ones) with the hot-key inputs."""
    cs = []
    for c in F.CASES:
        kw = {k: v for k, v in c.items() if k not in ("id", "mutants", "na")}
        cs.append(_case("form-" + c["id"], **kw))
    return cs


def _other_cases():
    cs = []
    # paged varlen: form_ref's packed lengths, both page sizes, both kernels the paged call can take (tfa_fwd_varlen_paged_variant) and its own choice
    for i, (D, dt, causal, page, var) in enumerate([(128, BF16, True, 64, 30), (128, FP16, False, 256, 32), (64, FP16, True, 256, 30), (64, BF16, False, 64, 32),
                                                    (96, BF16, True, 256, -1), (40, FP16, True, 64, -1)]):
        cs.append(_case(f"paged-d{D}-{'bf16' if dt == BF16 else 'fp16'}-{'c' if causal else 'f'}-p{page}-v{var if var >= 0 else 'auto'}", kind="paged", D=D, dtype=dt,
                        H=4, Hk=[2, 4, 1][i % 3], lq=F.VARLEN_LQ, lk=F.VARLEN_LK, causal=causal, page=page, variant=var, seed=2300 + i))
    # plain packed batches by kernel (the forms' six packed cases all carry a form)
    for i, (D, dt, causal, var) in enumerate([(128, BF16, True, 30), (64, FP16, False, 32), (96, FP16, True, -1), (40, BF16, False, -1)]):
        cs.append(_case(f"varlen-d{D}-{'bf16' if dt == BF16 else 'fp16'}-{'c' if causal else 'f'}-v{var if var >= 0 else 'auto'}", kind="varlen", D=D, dtype=dt, H=4,
                        Hk=[2, 1, 4][i % 3], lq=F.VARLEN_LQ, lk=F.VARLEN_LK, causal=causal, variant=var, seed=2350 + i))
    # split-KV: 2 and 3 chunks; rows that see no key at all and rows whose later chunks are empty (causal, Nq > Nk); D 128 (one launch) and 256 (one per chunk);
    # the one case above 450 keys: three chunks of at least two tiles
    for i, (D, dt, Nq, Nk, causal, splits, Hk) in enumerate([(128, BF16, 70, 203, False, 2, 2), (128, FP16, 257, 130, True, 2, 4), (64, BF16, 320, 385, True, 3, 1),
                                                             (256, FP16, 33, 385, False, 3, 2), (256, BF16, 70, 203, True, 2, 4), (128, BF16, 33, 700, True, 3, 2),
                                                             (96, FP16, 1, 300, False, 3, 1)]):
        cs.append(_case(f"splitkv-d{D}-{'bf16' if dt == BF16 else 'fp16'}-{'c' if causal else 'f'}-s{splits}-{Nq}x{Nk}", kind="splitkv", D=D, dtype=dt, Hk=Hk, Nq=Nq,
                        Nk=Nk, causal=causal, splits=splits, seed=2400 + i))
    # peaked rows (bf16; TFA_RULE_FIRST_TILE keeps the first tile's maximum): the dominant key in the THIRD tile, 20 nats above the rest in batch entry 0 (no
    # re-base) and 30 in entry 1 (the row sum passes 2^40 and re-bases); no other hot key, so that the first tile's maximum is an ordinary score
    # 257 rows: past the idle-wave instantiation of every forced variant (variant 30: Nq > 224), so that each runs its main one — the first-tile rule
    for var in (30, 32, 36, 37, -1):
        for causal in (False, True):
            cs.append(_case(f"peaked-v{var if var >= 0 else 'auto'}-{'c' if causal else 'f'}", D=128, dtype=BF16, B=2, Hk=2, Nq=257, Nk=320, causal=causal, variant=var,
                            peak=(20.0, 30.0), hot=False, seed=2500 + var + causal))
    # a head dim below the kernel width as a column slice of wider tensors: NaN in the other columns of q, k, v, a sentinel in out's
    cs.append(_case("sliced-d96-of-128-bf16", kind="sliced", D=96, Dfull=128, off=16, dtype=BF16, Hk=2, Nq=70, Nk=203, causal=True, seed=2600))
    cs.append(_case("sliced-d40-of-64-fp16", kind="sliced", D=40, Dfull=64, off=8, dtype=FP16, Hk=4, Nq=257, Nk=130, causal=False, seed=2601))
    return cs


CASES = _plain_cases() + _form_cases() + _other_cases()
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES), "case ids must be unique"


def _bhnd_cases():
    """The flat entry points tfa_fwd_bhnd / tfa_fwd_bhnd_f32out (tests/test_boundary_gpu.py) and the C host that calls them: contiguous (B,H,N,D), Hk = H,
    Nq = Nk, automatic variant — the smallest shapes that cross the second 256-row block (N 320), a head dim below the kernel's width (D 40, one row into the
    second block) and the 256-wide kernel (D 256).  A list of its own: the GPU parametrisation over CASES does not change."""
    cs = []
    for i, (dt, B, H, N, D, causal) in enumerate([(BF16, 2, 4, 320, 128, True), (FP16, 1, 2, 192, 64, False), (BF16, 1, 2, 257, 40, True),
                                                  (FP16, 1, 2, 200, 256, True)]):
        cs.append(_case(f"bhnd-{'bf16' if dt == BF16 else 'fp16'}-b{B}h{H}-d{D}-{'c' if causal else 'f'}-{N}", D=D, dtype=dt, B=B, H=H, Hk=H, Nq=N, Nk=N, causal=causal,
                        seed=2700 + i))
    return cs


BHND_CASES = _bhnd_cases()
# the fixed-length forward + backward problem tests/test_threads_gpu.py runs from several threads and streams (GQA, second blocks on both sides)
THREADS_CASE = _case("threads-bf16-h4hk2-d128-c-320x385", D=128, dtype=BF16, B=1, H=4, Hk=2, Nq=320, Nk=385, causal=True, seed=2710)
# ... and the split-KV problem of test_chunk_route_side_streams_and_graph_capture (head dim 256: one launch per key chunk over the calling thread's side streams)
THREADS_SPLITKV_CASE = _case("threads-splitkv-bf16-h8hk4-d256-c-s4-3x6000", kind="splitkv", D=256, dtype=BF16, B=1, H=8, Hk=4, Nq=3, Nk=6000, causal=True, splits=4,
                             seed=2711)
BOUNDARY_BY_ID = {c["id"]: c for c in BHND_CASES + [THREADS_CASE, THREADS_SPLITKV_CASE]}
assert not set(BOUNDARY_BY_ID) & set(BY_ID), "case ids must be unique"


def sweep_case(seed):
    """test_seeded_sweep's draw: dtype, D (a multiple of 8 up to 128; one draw in eight, fixed-length ones, from 136..256 without a form), G, B, Nq and Nk in
    1..450, fixed / packed / paged, a random legal form (form_ref.sweep_case's), a forced or the automatic variant."""
    r = random.Random(9000 + seed)
    base = F.sweep_case(seed)
    kw = {k: v for k, v in base.items() if k not in ("id", "mutants", "na")}
    wide = base["kind"] == "fixed" and r.random() < 0.19     # (packed calls stop at 128: one draw in eight overall)
    kind = "fixed" if base["kind"] == "fixed" else "varlen"
    plain = r.random() < 0.3
    if wide or plain:
        kw.update(window=(-1, -1), slopes=None, cap=0.0, std=0.5, bias=None)
    if wide:
        kw["D"] = 8 * r.randint(17, 32)
    formless = wide or plain
    if formless and kind == "varlen" and not wide and r.random() < 0.5:
        kind, kw["page"] = "paged", r.choice(PAGES)
    var = -1
    if not wide and r.random() < 0.5:
        form = kw["slopes"] is not None or kw["cap"] or kw["bias"] is not None or F.eff_window(kw["causal"], kw["window"]) not in ((-1, -1), (-1, 0))
        var = r.choice([30, 32]) if (form or kind != "fixed") else r.choice([30, 32, 36, 37, 17] + ([38] if kw["D"] in (64, 128) else []))
    kw.update(kind=kind, variant=var, layout=r.choice(["bhnd", "bnhd"]) if kind == "fixed" and kw["bias"] is None else "bhnd")
    return _case(f"sweep{seed}", **kw)


def case_of(case_id):
    if case_id in BOUNDARY_BY_ID:
        return BOUNDARY_BY_ID[case_id]
    return BY_ID[case_id] if case_id in BY_ID else sweep_case(int(case_id[len("sweep"):]))


# ---- the inputs: weight on the keys where indexing goes wrong -----------------------------------------------------------------------------------------
def hot_keys(c, Nq, Nk, cap=16):
    """The keys of one (Nq, Nk) problem where an indexing error lives, at most `cap` of them (interior tile seams are dropped first): for a handful of probe
    rows — row 0, the last row, the rows either side of the first 32-row wave, 128-row and 256-row block seam, the rows either side of the causal diagonal's
    first tile seam — the first and the last key the row sees and the first key beyond each edge; keys 63 / 64 / 127 / 128; the last key and the ragged tail's
    first; paged: the head row of the last page; split-KV: the last key of every chunk that has a successor."""
    if Nk == 0:
        return []
    left, right = F.eff_window(c["causal"], c["window"])
    shift = Nk - Nq
    rows = {0, Nq - 1}
    for seam in (32, 128, 256):
        if seam < Nq:
            rows |= {seam - 1, seam}
    if right >= 0:
        rows |= {r for r in (63 - right - shift, 64 - right - shift) if 0 <= r < Nq}
    must, edge = {0, Nk - 1}, set()
    if Nk % 64:
        must.add(Nk // 64 * 64)
    if c["page"]:
        must.add((Nk - 1) // c["page"] * c["page"])
    if c["kind"] == "splitkv":
        ch = K.chunk_of(Nk, c["splits"])
        must |= {s - 1 for s in range(ch, Nk, ch)}
    for i in sorted(rows):
        lo = 0 if left < 0 else i + shift - left
        hi = Nk - 1 if right < 0 else i + shift + right
        edge |= {j for j in (lo - 1, lo, hi, hi + 1) if 0 <= j < Nk and (left >= 0 or right >= 0)}
    seams = {j for j in (63, 64, 127, 128) if j < Nk}
    hot = sorted(must)
    for group in (sorted(edge - must), sorted(seams - must - edge)):
        hot += group[:max(0, cap - len(hot))]
    return sorted(hot)


def _heat(c, k, Nq, Nk, e, sc, peak=None):
    """Adds beta * e to the hot keys of one sequence's K (Hk, Nk, D) fp32, in place: beta such that the hot keys together hold about half of a row's probability
    (kvcache_ref.build's rule: exp(bump) = 1.6 * cold keys / hot keys).  peak: the dominant key (150, the third tile) that many nats above the rest instead."""
    if peak is not None:
        k[:, 150] += peak / (sc * ALPHA) * e
        return
    hot = hot_keys(c, Nq, Nk) if c["hot"] else []
    if hot:
        bump = max(1.0, math.log(max(Nk - len(hot), 1) / len(hot)) + 0.5)
        for j in hot:
            k[:, j] += bump / (sc * ALPHA) * e


def build(case, dtype=None):
    """The tensors of a case, on the CPU: form_ref.build's (q, k, v, form, slopes, bias, cu_q, cu_k, sc) with the hot-key inputs — every q row gets a component
    ALPHA along one unit direction e, the hot_keys of every sequence get beta * e (see _heat) — so that a single dropped, added or misplaced key moves out and lse
    by percents at any length.  Rows outside every sequence (packed) and behind the lengths and in spare pages (paged): finite garbage of std 3 whose first key
    is hot, never NaN (test_isolation and its siblings own the NaN cases).  paged: k_pool / v_pool (num_pages, page, Hk, D) under a permuted block table `bt`
    with three spare pages; the logical keys are READ BACK through kvcache_ref.gather.  sliced: q_full, k_full, v_full (D = Dfull, NaN outside the slice)."""
    c = case
    t = F.build(dict(c, kind="varlen" if packed(c) else "fixed"), dtype)
    t["case"] = c
    dt, sc, D, Hk = t["dtype"], t["sc"], c["D"], c["Hk"]
    g = torch.Generator().manual_seed(5000 + c["seed"])
    e = (torch.randint(0, 2, (D,), generator=g).float() * 2 - 1) / math.sqrt(D)
    t["e"] = e
    q, k = t["q"].float() + ALPHA * e, t["k"].float()
    if packed(c):
        ck, cq = t["cu_k"], t["cu_q"]
        for b, (nq, nk) in enumerate(shapes_of(c)):
            _heat(c, k[int(ck[b]):int(ck[b + 1])].transpose(0, 1), nq, nk, e, sc)
        tail = int(ck[-1])
        k[tail:] = torch.randn(k[tail:].shape, generator=g) * 3.0
        k[tail] += 4.0 / (sc * ALPHA) * e
        v = t["v"].float()
        v[tail:] = torch.randn(v[tail:].shape, generator=g) * 3.0
        t["v"] = v.to(dt)
    else:
        for b in range(c["B"]):
            _heat(c, k[b], c["Nq"], c["Nk"], e, sc, None if c["peak"] is None else c["peak"][b])
    t["q"], t["k"] = q.to(dt), k.to(dt)
    if c["kind"] == "paged":
        _paginate(t, g)
    if c["kind"] == "sliced":
        for n in ("q", "k", "v"):
            full = torch.full(t[n].shape[:-1] + (c["Dfull"],), math.nan, dtype=dt)
            full[..., c["off"]:c["off"] + D] = t[n]
            t[n + "_full"] = full
    return t


def _paginate(t, g):
    """The logical keys of a packed batch into a pool of pages under a permuted table: three spare pages and every row behind a length hold garbage of std 3, the
    first row behind a length hot; table entries behind a sequence's pages name a spare page."""
    c, dt = t["case"], t["dtype"]
    page, Hk, D = c["page"], c["Hk"], c["D"]
    need = [(n + page - 1) // page for n in c["lk"]]
    used = sum(need)
    num = used + 3
    perm = torch.randperm(num, generator=g).tolist()
    assert perm[:used] != list(range(used)), "the table must not be the identity"
    kp, vp = (torch.randn(num, page, Hk, D, generator=g) * 3.0 for _ in range(2))
    bt = torch.full((len(need), max(need) + 1), perm[used], dtype=torch.int32)
    nxt = 0
    for b, n in enumerate(c["lk"]):
        k0 = int(t["cu_k"][b])
        for i in range(need[b]):
            pg = perm[nxt]
            nxt += 1
            bt[b, i] = pg
            rows = min(page, n - i * page)
            kp[pg, :rows] = t["k"][k0 + i * page:k0 + i * page + rows].float()
            vp[pg, :rows] = t["v"][k0 + i * page:k0 + i * page + rows].float()
            if rows < page:
                kp[pg, rows] += 4.0 / (t["sc"] * ALPHA) * t["e"]
    t["k_pool"], t["v_pool"], t["bt"] = kp.to(dt), vp.to(dt), bt


def parts(t):
    """A case as {key: part}: {None: the problem} or {b: sequence b} for every sequence with rows AND keys — part = dict(q, k, v as (1|B, H|Hk, n, D) views, form,
    Nq, Nk, and what the mutants read: k1 / v1 (one more key row), k_pn / v_pn (paged: the last page from the next sequence's table row), slopes_b0)."""
    c = t["case"]
    res = {}
    if not packed(c):
        p = dict(q=t["q"], k=t["k"], v=t["v"], form=t["form"], Nq=c["Nq"], Nk=c["Nk"])
        if c["slopes"] == "BH":
            p["slopes_b0"] = t["slopes"][0:1].expand_as(t["slopes"]).contiguous()
        return {None: p}
    B = t["B"]
    for b in range(B):
        nq, nk = c["lq"][b], c["lk"][b]
        if nq == 0 or nk == 0:
            continue
        p = dict(q=F.seq_view(t["q"], t["cu_q"], b), form=F.seq_form(t["form"], b), Nq=nq, Nk=nk)
        if c["slopes"] == "BH":
            p["slopes_b0"] = t["slopes"][0]
        if c["kind"] == "paged":
            view = lambda x: x.transpose(0, 1).unsqueeze(0)      # noqa: E731  ((n, Hk, D) -> (1, Hk, n, D))
            cap = t["bt"].shape[1] * c["page"]
            p["k"], p["v"] = (view(K.gather(x, t["bt"], b, nk)) for x in (t["k_pool"], t["v_pool"]))
            p["k1"], p["v1"] = (view(K.gather(x, t["bt"], b, min(nk + 1, cap))) for x in (t["k_pool"], t["v_pool"]))
            p["k_pn"], p["v_pn"] = (view(K.gather(x, t["bt"], b, nk, (b + 1) % B)) for x in (t["k_pool"], t["v_pool"]))
        else:
            p["k"], p["v"] = F.seq_view(t["k"], t["cu_k"], b), F.seq_view(t["v"], t["cu_k"], b)
            p["k1"], p["v1"] = F.seq_view(t["k"], t["cu_k"], b, 1), F.seq_view(t["v"], t["cu_k"], b, 1)
        res[b] = p
    return res


def reference(t):
    """{key: (out64, lse64, A, T, lse bound)} of every part: the definition (form_ref.ref_fwd) and the bounds' magnitudes."""
    c = t["case"]
    res = {}
    for key, p in parts(t).items():
        out, lse, A = F.ref_fwd(p["q"], p["k"], p["v"], t["sc"], **p["form"])
        T = bound_terms(p["q"], p["k"], t["sc"], **p["form"])
        bound = lse_bound(T, p["Nk"], torch.where(torch.isfinite(lse), lse, torch.zeros_like(lse)), c["D"], splits=c["splits"], slopes=c["slopes"] is not None,
                          bias=c["bias"] is not None, cap=c["cap"])
        res[key] = (out, lse, A, T, bound)
    return res


def rnd_twin(t):
    """The case's tensors with form_ref.rnd inputs of the same shapes (what the suite's other forward tests draw): for the record of what the OLD bars let through."""
    c = t["case"]
    t2 = F.build(dict(c, kind="varlen" if packed(c) else "fixed"), t["dtype"])
    t2["case"] = c
    if c["kind"] == "paged":
        t2["e"] = torch.zeros(c["D"])
        _paginate(t2, torch.Generator().manual_seed(5000 + c["seed"]))
    return t2
