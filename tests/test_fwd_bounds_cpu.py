"""CPU proof that the per-element bounds of tests/fwd_ref.py are the right size for every case tests/test_fwd_bounds_gpu.py runs:
  1. one definition: fwd_ref.attend without a defect IS form_ref.ref_fwd (1e-12), which without a form IS oracle.exact64 / abs_weighted (2^-23: the C oracle
     returns fp32);
  2. the correct algorithm fits: a 16-bit emulation of the kernels' algorithm — fp32 scores, P rounded to 16 bits against every row reference the library
     has (oracle.tiled_emulation / _lazy / _first_tile / ksplit_emulation; for the forms a score-matrix-driven restatement of the same loops, checked against
     those four at "no form"), fp32 sums, the chunks' merge, O rounded once — stays below 1.0 of the fp32 out bound, of the 16-bit out bound and of the LSE
     bound on every element, in both dtypes, on every case of the GPU list and every draw of its seeded sweep — and on the cases of the flat entry points
     (tests/test_boundary_gpu.py) and of the thread test (tests/test_threads_gpu.py), fwd_ref.BOUNDARY_BY_ID;
  3. the bounds bite: every mutant a case names (fwd_ref.MUTANTS) misses the out bound or the LSE bound by at least 10x in some element; every mutant is named
     by at least two cases; a mutant a case does not name is in its `na` with a structural reason; every sweep draw has a mutant that bites;
  4. on the record (printed, not asserted; profiles/fwd_bounds.txt): which (case, mutant) pairs the bars the suite asserted before — 1e-2 on the 16-bit out,
     eps16 * A + 1e-6 on the fp32 out, 1e-4 on the LSE (the forms: 1e-4 * max(1, |lse|)) — let through, on these inputs and on form_ref.rnd inputs of the same shapes; and the size
     of the LSE bound next to the old bar.
No GPU, no kernel: fp64 and fp32 on the host.
"""
import functools
import math

import pytest
import torch

import form_ref as F
import fwd_ref as R
import kvcache_ref as K

IDS = [c["id"] for c in R.CASES]
BHND_IDS = list(R.BOUNDARY_BY_ID)   # the flat entry points' cases (tests/test_boundary_gpu.py) and the threads' forward problem (tests/test_threads_gpu.py)
SWEEP = [f"sweep{s}" for s in range(48)]
BITE = 10.0
LN2 = 0.6931471805599453
f32 = torch.float32


@functools.lru_cache(maxsize=None)
def _reference(case_id, dtype):
    """(tensors, parts, fp64 reference per part) of a case in `dtype`: computed once, shared by the tests below."""
    t = R.build(R.case_of(case_id), dtype)
    return t, R.parts(t), R.reference(t)


# ---- the score-matrix-driven emulation ------------------------------------------------------------------------------------------------------------
def _group_any(x, group):
    B, H, Nq, _ = x.shape
    ngrp = (Nq + group - 1) // group
    og = torch.nn.functional.pad(x, (0, 0, 0, ngrp * group - Nq)).view(B, H, ngrp, group).any(dim=-1, keepdim=True)
    return og.expand(B, H, ngrp, group).reshape(B, H, ngrp * group, 1)[:, :, :Nq]


def emulate_scores(raw, v, sc, dtype, rule, tiles=None):
    """The il kernels' tile loop on a given matrix of RAW fp32 scores (B,H,Nq,Nk) (the cap, the ALiBi and bias terms and the mask already in, -inf = masked, as
    apply_bias / apply_mask leave them in front of the loop): oracle.tiled_emulation_lazy's statements — rule "exact" is its thresh = 0, group = 1 — and
    tiled_emulation_first_tile's without the redo pass (asserted not to be needed).  tiles: the key indices of each 64-key tile (a wave group's, a chunk's).
    Returns (out fp32 unrounded, lse fp32)."""
    B, H, Nq, Nk = raw.shape
    tiles = [torch.arange(s, min(s + 64, Nk)) for s in range(0, Nk, 64)] if tiles is None else tiles
    sc2 = torch.tensor(sc * R.LOG2E, dtype=f32)
    thresh, group = (0.0, 1) if rule == "exact" else (8.0, 32)
    acc = torch.zeros((B, H, Nq, v.shape[-1]), dtype=f32)
    l = torch.zeros((B, H, Nq, 1), dtype=f32)
    ref = torch.full((B, H, Nq, 1), -1e30, dtype=f32)
    for ti, idx in enumerate(tiles):
        s = raw[..., idx]
        xm = s.max(dim=-1, keepdim=True).values * sc2
        if rule == "first_tile":
            if ti == 0:
                ref = torch.maximum(ref, xm)
        else:
            trig = _group_any(xm > ref + thresh, group)
            nref = torch.where(trig, torch.maximum(ref, xm), ref)
            alpha = torch.exp2(ref - nref)
            l, acc, ref = l * alpha, acc * alpha, nref
        pr = torch.exp2((s.double() * sc2.double() - ref.double()).float())
        l = l + pr.sum(dim=-1, keepdim=True)
        acc = acc + torch.matmul(pr.to(dtype).float(), v[:, :, idx])
        if rule == "first_tile":
            assert bool((l <= 2.0 ** 64).all()), "a redone block: use oracle.tiled_emulation_first_tile"
            trig = _group_any(l > 2.0 ** 40, group)
            if bool(trig.any()):
                e = torch.where(trig, torch.floor(torch.log2(torch.where(l > 0, l, torch.ones_like(l)))).clamp(0, 126), torch.zeros_like(l))
                a = torch.exp2(-e)
                l, acc, ref = l * a, acc * a, ref + e
    empty = l == 0
    out = torch.where(empty, torch.zeros_like(acc), acc / torch.where(empty, torch.ones_like(l), l))
    lse = torch.where(empty, torch.full_like(l, math.inf), (ref + torch.log2(torch.where(empty, torch.ones_like(l), l))) * LN2).squeeze(-1)
    return out, lse


def merge32(outs, lses):
    """tfa_merge.hip / the key-split epilogue in fp32: m = max of the parts' LSEs, w = exp(l - m), out = sum w o / sum w, lse = m + log sum w; +inf = empty."""
    ls = torch.stack(lses)
    fin = torch.isfinite(ls)
    neg = torch.where(fin, ls, torch.full_like(ls, -math.inf))
    m = neg.max(dim=0).values
    w = torch.where(fin, torch.exp(neg - torch.where(torch.isfinite(m), m, torch.zeros_like(m))), torch.zeros_like(ls))
    ws = w.sum(0)
    out = (w.unsqueeze(-1) * torch.stack(outs)).sum(0) / torch.where(ws > 0, ws, torch.ones_like(ws)).unsqueeze(-1)
    return out, torch.where(ws > 0, m + torch.log(torch.where(ws > 0, ws, torch.ones_like(ws))), torch.full_like(ws, math.inf))


def _ksplit_tiles(Nk):
    nt = (Nk + 63) // 64
    return [[torch.arange(t * 64, min((t + 1) * 64, Nk)) for t in range(g, nt, 2)] for g in (0, 1) if g < nt]


def _raw_scores(q, k, sc, **form):
    """The raw-domain fp32 scores of a form: the fp64 definition's scores (form_ref.scores64: cap, ALiBi, bias, mask) divided by the scale."""
    s, _ = F.scores64(F._f64(q), F._expand_kv(F._f64(k), q.shape[1]), sc, **form)
    return (s / sc).float()


def _plain_raw(q, k, causal):
    """oracle.tiled_emulation_lazy's scores, bit for bit: fp32 matmuls tile by tile, the causal mask bottom-right aligned."""
    qf, kf = q.float(), F._expand_kv(k.float(), q.shape[1])
    Nq, Nk = q.shape[2], k.shape[2]
    rows = torch.arange(Nq)[:, None] + (Nk - Nq)
    out = []
    for s0 in range(0, Nk, 64):
        s = torch.matmul(qf, kf[:, :, s0:s0 + 64].transpose(2, 3))
        if causal:
            s = s.masked_fill((s0 + torch.arange(s.shape[-1]))[None, :] > rows, -math.inf)
        out.append(s)
    return torch.cat(out, dim=-1)


def emulations(oracle, case, part, sc, dtype):
    """[(name, out fp32 unrounded, lse fp32)]: the problem of one part under every row reference and merge the library could run it with."""
    c = case
    q, k, v = part["q"], part["k"], part["v"]
    left, right = part["form"]["window"]
    formless = c["slopes"] is None and not c["cap"] and c["bias"] is None and (left, right) in ((-1, -1), (-1, 0))
    res = []
    if not formless:                                        # the forms: TFA_RULE_LAZY for both dtypes; the exact rule for good measure
        raw, vf = _raw_scores(q, k, sc, **part["form"]), F._expand_kv(v.float(), q.shape[1])
        for rule in ("lazy", "exact"):
            res.append((rule,) + emulate_scores(raw, vf, sc, dtype, rule))
        return res
    causal = right == 0
    Nk = k.shape[2]
    if c["kind"] == "splitkv":                              # per chunk: the LDS-DMA kernel (exact maximum; D > 128: the x4 kernel, lazy), then tfa_merge
        for rule, kw in (("exact", dict(group=1, thresh=0.0)), ("lazy", {})):
            po = [oracle.tiled_emulation_lazy(q, k[:, :, lo:hi], v[:, :, lo:hi], causal, sc, p_dtype=dtype, return_lse=True, key_pos=torch.arange(lo, hi),
                                              nk_total=Nk, **kw) for lo, hi in K._chunks(Nk, c["splits"]) if hi > lo]
            res.append((f"chunks-{rule}",) + merge32([o for o, _ in po], [l for _, l in po]))
        return res
    res.append(("exact",) + oracle.tiled_emulation(q, k, v, causal, sc, p_dtype=dtype, return_lse=True))
    res.append(("lazy",) + oracle.tiled_emulation_lazy(q, k, v, causal, sc, p_dtype=dtype, return_lse=True))
    res.append(("ksplit-lazy",) + oracle.ksplit_emulation(q, k, v, causal, sc, return_lse=True, p_dtype=dtype))
    if dtype == torch.bfloat16:
        res.append(("first-tile",) + oracle.tiled_emulation_first_tile(q, k, v, causal, sc, p_dtype=dtype, return_lse=True))
        res.append(("ksplit-first-tile",) + oracle.ksplit_emulation(q, k, v, causal, sc, return_lse=True, rule="first_tile", p_dtype=dtype))
    return res


# ---- 1. one definition --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("B,H,Hk,Nq,Nk,D", [(2, 4, 2, 96, 96, 64), (1, 4, 1, 70, 203, 40), (1, 2, 2, 257, 130, 128), (2, 3, 3, 33, 65, 72)])
def test_no_form_is_the_existing_oracle(oracle, causal, B, H, Hk, Nq, Nk, D):
    c = R._case("plain", dtype=torch.bfloat16, B=B, H=H, Hk=Hk, D=D, Nq=Nq, Nk=Nk, causal=causal, seed=77)
    t = R.build(c)
    p = R.parts(t)[None]
    out, lse, A, T, _ = R.reference(t)[None]
    o64, l64 = oracle.exact64(t["q"], t["k"], t["v"], causal, t["sc"], return_lse=True)
    a64 = oracle.abs_weighted(t["q"], t["k"], t["v"], causal, t["sc"])
    for mine, them in ((out, o64), (A, a64)):
        assert (mine - them.double()).abs().max().item() <= 2.0 ** -23 * them.abs().max().item() + 1e-12
    seen = torch.isfinite(lse)
    assert bool(seen.all()) == (not causal or Nk >= Nq) and torch.equal(~seen, F.structure(t["q"], t["k"], t["sc"], **t["form"])[0])
    assert (lse[seen] - l64.double()[seen]).abs().max().item() <= 2.0 ** -22 * max(1.0, l64[seen].abs().max().item())
    mo, ml = R.attend(p, t["sc"])                           # the mutants' function without a defect: form_ref.ref_fwd, fp64 throughout
    assert (mo - out).abs().max().item() <= 1e-12 * out.abs().max().item() and torch.equal(torch.isposinf(ml), ~seen)
    assert (ml[seen] - lse[seen]).abs().max().item() <= 1e-12 * lse[seen].abs().max().item()
    assert bool((T[seen] >= lse[seen].abs() - math.log(Nk) - 1e-9).all()), "T bounds every visible score, so |lse| <= T + ln n"


@pytest.mark.parametrize("case_id", ["form-win37_20-320x385", "form-alibi-BH-1_-1-320x385", "form-cap5-std2-BH-c-1_-1-70x203", "form-bias-BH-q-inf-contig-1_-1-192x192",
                                     "form-varlen-w100_0-BH-cap5", "paged-d128-bf16-c-p64-v30", "splitkv-d64-bf16-c-s3-320x385"])
def test_attend_without_a_defect_is_the_definition(case_id):
    t, parts, ref = _reference(case_id, R.BY_ID[case_id]["dtype"])
    for key, p in parts.items():
        out, lse = ref[key][:2]
        mo, ml = R.attend(p, t["sc"], None, t["case"]["splits"])
        fin = torch.isfinite(lse)
        assert torch.equal(torch.isposinf(ml), ~fin) and (mo - out).abs().max().item() <= 1e-12 * max(out.abs().max().item(), 1e-30)
        assert (ml[fin] - lse[fin]).abs().max().item() <= 1e-12 * max(lse[fin].abs().max().item(), 1.0)


@pytest.mark.parametrize("causal", [False, True])
def test_score_driven_emulation_is_the_oracles(oracle, causal):
    """emulate_scores at "no form" against the four loops it restates: the lazy, the first-tile and the key-split one to fp32 round-off (the same statements on
    the same scores; the oracle's merge takes a logsumexp where merge32 takes max and sum), the reference's own loop (natural exponentials against the running
    maximum: the same rounding points, other fp32 operations) within a flipped rounding of single P values."""
    q, k, v = F.rnd((1, 3, 200, 64), torch.bfloat16, 5), F.rnd((1, 3, 330, 64), torch.bfloat16, 6), F.rnd((1, 3, 330, 64), torch.bfloat16, 7)
    k[:, :, 150] *= 4.0
    sc, dt = 0.125, torch.bfloat16
    raw, vf = _plain_raw(q, k, causal), v.float()
    A = oracle.abs_weighted(q, k, v, causal, sc).double()
    close = lambda a, b: (a.double() - b.double()).abs().max().item() <= 2.0 ** -20 * max(1.0, b.abs().max().item())     # noqa: E731
    for rule, them in (("lazy", oracle.tiled_emulation_lazy(q, k, v, causal, sc, return_lse=True)),
                       ("first_tile", oracle.tiled_emulation_first_tile(q, k, v, causal, sc, return_lse=True))):
        o, l = emulate_scores(raw, vf, sc, dt, rule)
        assert close(o, them[0]) and close(l, them[1]), rule
    parts = [emulate_scores(raw, vf, sc, dt, "lazy", tiles) for tiles in _ksplit_tiles(330)]
    o, l = merge32([p[0] for p in parts], [p[1] for p in parts])
    them = oracle.ksplit_emulation(q, k, v, causal, sc, return_lse=True)
    assert close(o, them[0]) and close(l, them[1]), "key split"
    o, l = emulate_scores(raw, vf, sc, dt, "exact")
    them = oracle.tiled_emulation(q, k, v, causal, sc, return_lse=True)
    d = (o.double() - them[0].double()).abs()
    assert bool((d <= 2.0 ** -8 * A + 1e-6).all()) and d.median().item() <= 1e-6 and close(l, them[1]), "exact maximum"
    # ... and the raw scores of a form, through the fp64 definition, are the matmul's at "no form" (to fp32 round-off of a score)
    s2 = _raw_scores(q, k, sc, window=(-1, 0) if causal else (-1, -1))
    fin = torch.isfinite(raw)
    assert torch.equal(fin, torch.isfinite(s2)) and (raw[fin] - s2[fin]).abs().max().item() <= 2.0 ** -20 * raw[fin].abs().max().item()


# ---- 2. the correct algorithm fits --------------------------------------------------------------------------------------------------------------------
def _fit(oracle, case_id, dtype):
    t, parts, ref = _reference(case_id, dtype)
    w = {"out32": 0.0, "out16": 0.0, "lse": 0.0}
    who = dict(w)
    for key, p in parts.items():
        out, lse, A, T, bound = ref[key]
        for name, o32, l32 in emulations(oracle, t["case"], p, t["sc"], dtype):
            got = {"out32": R.out_ratio(o32.double(), out, A, dtype, False), "out16": R.out_ratio(F.round16(o32, dtype), out, A, dtype, True),
                   "lse": R.lse_ratio(l32, lse, bound)}
            for n, r in got.items():
                if r > w[n]:
                    w[n], who[n] = r, name
    return w, who


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case_id", IDS + BHND_IDS + SWEEP)
def test_emulation_fits(oracle, case_id, dtype):
    w, who = _fit(oracle, case_id, dtype)
    print(f"{case_id}: emulation at {w['out32']:.3f} of the fp32 out bound ({who['out32']}), {w['out16']:.3f} of the 16-bit one ({who['out16']}), "
          f"{w['lse']:.4f} of the LSE bound ({who['lse']})")
    assert max(w.values()) <= 1.0


# ---- 3. the bounds bite -----------------------------------------------------------------------------------------------------------------------------------
def test_every_case_names_its_mutants():
    for c in R.CASES + [R.sweep_case(s) for s in range(48)]:
        assert c["mutants"], c["id"]
        assert set(c["mutants"]) | {m for m, _ in c["na"]} == set(R.MUTANTS) and not set(c["mutants"]) & {m for m, _ in c["na"]}, c["id"]
        assert all(why for _, why in c["na"]), c["id"]
    for m in R.MUTANTS:
        assert sum(1 for c in R.CASES if m in c["mutants"]) >= 2, f"{m} is named by fewer than two cases"


def test_the_case_list_covers_the_minimum():
    """What the GPU file must cover, asserted on the list itself so that it cannot shrink unnoticed — and the caps that keep it quick."""
    cs = R.CASES
    G = lambda c: c["H"] // c["Hk"]                      # noqa: E731
    plain = [c for c in cs if c["id"].startswith("plain-d")]
    for D in (40, 64, 96, 128):                          # every product variant up to 128 wide, forced, and the automatic choice; both dtypes, causal and not
        for var in (-1, 30, 32, 36, 37, 38, 17):
            got = [c for c in plain if c["D"] == D and c["variant"] == var]
            assert {c["dtype"] for c in got} == {R.BF16, R.FP16} and {c["causal"] for c in got} == {False, True}, (D, var)
    # ... and each forced il variant in its PRODUCT instantiation (main; narrow for il8 / il4 at D 96), not only the idle-wave one small blocks run: both dtypes
    for D in (40, 64, 96, 128):
        for var in (30, 32, 36, 37, 38):
            got = {c["dtype"] for c in plain if c["D"] == D and c["variant"] == var and R.il_instantiation(var, c["Nq"], D) == ("narrow" if D == 96 and var in (30, 32) else "main")}
            assert got == {R.BF16, R.FP16}, (D, var, got)
    assert {c["dtype"] for c in plain if c["D"] == 136} == {c["dtype"] for c in plain if c["D"] == 256} == {R.BF16, R.FP16}
    assert {(c["Nq"], c["Nk"]) for c in plain} == set(R.PLAIN_SHAPES) and set(R.PLAIN_SHAPES) >= set(F.SHAPES) | {(1, 300), (33, 65)}
    assert {G(c) for c in plain} == {1, 2, 4} and {c["layout"] for c in plain} == {"bhnd", "bnhd"}
    assert any(R.packs_gqa(c) and c["causal"] and (c["Nq"], c["Nk"], c["H"], c["Hk"]) == (4, 200, 8, 2) for c in cs), "packed GQA rows with positions"
    forms = [c for c in cs if c["id"].startswith("form-")]
    assert [c["id"][5:] for c in forms] == [c["id"] for c in F.CASES], "form_ref.CASES' form parameters, all of them"
    assert all({k: v for k, v in c.items() if k in f and k not in ("id", "mutants", "na")} == {k: v for k, v in f.items() if k not in ("id", "mutants", "na")}
               for c, f in zip(forms, F.CASES))
    pk = [c for c in cs if R.packed(c)]
    assert all(c["lq"] == F.VARLEN_LQ and c["lk"] == F.VARLEN_LK for c in pk) and F.VARLEN_TAIL[0] > 0
    pg = [c for c in cs if c["kind"] == "paged"]
    assert {c["page"] for c in pg} == set(R.PAGES) and {c["variant"] for c in pg} == {-1, 30, 32}
    sk = [c for c in cs if c["kind"] == "splitkv"]
    assert {c["splits"] for c in sk} == {2, 3} and {128, 256} <= {c["D"] for c in sk}
    assert any(c["causal"] and c["Nq"] > c["Nk"] for c in sk), "rows whose every chunk, and rows whose later chunks, are empty"
    assert any(c["Nk"] >= 3 * 128 + 256 and c["splits"] == 3 for c in sk), "three chunks of at least two tiles"
    assert sum(1 for c in cs if max(nk for _, nk in R.shapes_of(c)) > 450) == 1 and all(max(nq for nq, _ in R.shapes_of(c)) <= 450 for c in cs)
    pe = [c for c in cs if c["peak"] is not None]
    assert {c["variant"] for c in pe} == {30, 32, 36, 37, -1} and all(c["dtype"] == R.BF16 and c["peak"] == (20.0, 30.0) and c["Nk"] > 192 for c in pe)
    assert all(R.il_instantiation(c["variant"], c["Nq"], c["D"]) == "main" for c in pe if c["variant"] >= 0), "every forced peaked case in its main instantiation"
    sl = [c for c in cs if c["kind"] == "sliced"]
    assert sl and all(c["off"] % 8 == 0 and c["off"] > 0 and c["Dfull"] > c["off"] + c["D"] - 1 and c["D"] not in (64, 128) for c in sl)
    sw = [R.sweep_case(s) for s in range(48)]
    assert {c["kind"] for c in sw} == {"fixed", "varlen", "paged"} and any(c["D"] > 128 for c in sw) and any(c["variant"] >= 0 for c in sw)


def _library_rule(c):
    """tfa_fwd_rounding_rule for the case's sizes under its forced variant (a host-side answer: no GPU)."""
    from tiny_flash_attention_amd import _lib

    _lib.set_variant(c["variant"])
    try:
        return _lib.rule_for(c["B"], c["H"], c["Hk"], c["Nq"], c["Nk"], c["D"], c["causal"], _lib.TFA_BF16 if c["dtype"] == R.BF16 else _lib.TFA_F16)
    finally:
        _lib.set_variant(-1)


def test_the_library_agrees_on_the_rounding_rules():
    """The library's own answer (tfa_fwd_rounding_rule) for the cases that are in the list FOR a rule: every peaked case — the four forced variants and the
    automatic choice — runs TFA_RULE_FIRST_TILE, and a forced il variant of the plain list runs it exactly where fwd_ref.il_instantiation says "main" in bf16."""
    from tiny_flash_attention_amd import _lib

    for c in R.CASES:
        if c["peak"] is not None:
            assert _library_rule(c) == _lib.RULE_FIRST_TILE, c["id"]
        elif c["id"].startswith("plain-d") and c["variant"] in (30, 32, 36, 37):
            first = c["dtype"] == R.BF16 and R.il_instantiation(c["variant"], c["Nq"], c["D"]) == "main"
            assert (_library_rule(c) == _lib.RULE_FIRST_TILE) == first, c["id"]
    first = {(c["D"], c["variant"]) for c in R.CASES if c["id"].startswith("plain-d") and c["variant"] >= 0 and _library_rule(c) == _lib.RULE_FIRST_TILE}
    assert first >= {(D, v) for D in (64, 128) for v in (30, 32, 36, 37)}, "the first-tile rule of every variant that has it, at both kernel widths"


def test_the_hot_keys_sit_where_the_issue_puts_them():
    c = R.BY_ID["plain-pack-bf16-4x200"]
    assert {0, 199, 192} <= set(R.hot_keys(c, 4, 200)) and {196, 197} <= set(R.hot_keys(c, 4, 200))      # row 0's last key and the first beyond
    c = R.BY_ID["splitkv-d128-bf16-c-s3-33x700"]
    assert {255, 511, 699, 640} <= set(R.hot_keys(c, 33, 700)) and len(R.hot_keys(c, 33, 700)) <= 16
    c = R.BY_ID["paged-d128-bf16-c-p64-v30"]
    assert {0, 299, 256} <= set(R.hot_keys(c, 300, 300))
    for c in R.CASES:
        for nq, nk in R.shapes_of(c):
            h = R.hot_keys(c, nq, nk)
            assert len(h) <= 16 and all(0 <= j < nk for j in h) and (nk == 0 or {0, nk - 1} <= set(h)), c["id"]


def _mutant_ratios(t, parts, ref, mutant, dtype):
    """(out against the 16-bit bound, lse against its bound), and what the bars the suite had before make of the same mutant: (16-bit out / 1e-2, fp32 out /
    (eps16 * A + 1e-6), lse / (1e-4 * max(1, |lse|)))."""
    wo = wl = 0.0
    old = [0.0, 0.0, 0.0]
    for key, p in parts.items():
        out, lse, A, _, bound = ref[key]
        mo, ml = R.attend(p, t["sc"], mutant, t["case"]["splits"])
        wo, wl = max(wo, R.out_ratio(mo, out, A, dtype, True)), max(wl, R.lse_ratio(ml, lse, bound))
        old = [max(a, b) for a, b in zip(old, (R.old_out_ratio(F.round16(mo, dtype), out), R.out_ratio(mo, out, A, dtype, False),
                                               R.lse_ratio(ml, lse, R.old_lse_bar(torch.where(torch.isfinite(lse), lse, torch.zeros_like(lse)), R.has_form(t["case"])))))]
    return wo, wl, old


@pytest.mark.parametrize("case_id,mutant", [(c["id"], m) for c in R.CASES + list(R.BOUNDARY_BY_ID.values()) for m in c["mutants"]])
def test_mutant_misses_a_bound(case_id, mutant):
    dtype = R.case_of(case_id)["dtype"]
    wo, wl, _ = _mutant_ratios(*_reference(case_id, dtype), mutant, dtype)
    print(f"{case_id} / {mutant}: misses the out bound by {wo:.1f}x, the LSE bound by {wl:.1f}x")
    assert max(wo, wl) >= BITE, f"{case_id}: mutant {mutant} is only {wo:.2f}x / {wl:.2f}x outside the bounds — the case's inputs do not tell it from the definition"


@pytest.mark.parametrize("seed", range(48))
def test_a_mutant_misses_a_bound_on_every_draw(seed):
    c = R.sweep_case(seed)
    got = {m: max(_mutant_ratios(*_reference(c["id"], c["dtype"]), m, c["dtype"])[:2]) for m in c["mutants"]}
    print(f"{c['id']}: " + "  ".join(f"{m} {r:.1f}x" for m, r in got.items()))
    assert got and max(got.values()) >= BITE, f"{c}: no mutant is 10x outside the bounds"


# ---- 4. on the record --------------------------------------------------------------------------------------------------------------------------------------
def test_the_old_bars_on_the_record():
    """Which (case, mutant) pairs each bar lets through BY ITSELF (the worst element at or below 1.0 of it), per mutant: the two new bounds on the hot-key inputs,
    and the three bars asserted before — 1e-2 on the 16-bit out, the only guard of the 16-bit epilogues; eps16 * A + 1e-6 on the fp32 out; 1e-4 (the forms: * max(1, |lse|)) on the LSE —
    on the hot-key inputs and on form_ref.rnd inputs of the same shapes, and all three together.  Printed for profiles/fwd_bounds.txt; the only assertion is
    that the two new bounds together let no pair through."""
    cols = ("new out16", "new lse", "new both", "hot: 1e-2", "hot: fp32", "hot: lse", "hot: all 3", "rnd: 1e-2", "rnd: fp32", "rnd: lse", "rnd: all 3")
    rows = {m: [0] * (1 + len(cols)) for m in R.MUTANTS}
    for c in R.CASES:
        t, parts, ref = _reference(c["id"], c["dtype"])
        t2 = R.rnd_twin(t)
        parts2, ref2 = R.parts(t2), R.reference(t2)
        for m in c["mutants"]:
            wo, wl, old = _mutant_ratios(t, parts, ref, m, c["dtype"])
            _, _, old2 = _mutant_ratios(t2, parts2, ref2, m, c["dtype"])
            got = [wo <= 1.0, wl <= 1.0, max(wo, wl) <= 1.0] + [x <= 1.0 for x in old] + [max(old) <= 1.0] + [x <= 1.0 for x in old2] + [max(old2) <= 1.0]
            rows[m][0] += 1
            for i, g in enumerate(got):
                rows[m][1 + i] += bool(g)
    print(f"{'mutant':13s} {'pairs':>5s} " + " ".join(f"{n:>10s}" for n in cols) + "      (pairs a bar lets through by itself)")
    for m, r in rows.items():
        print(f"{m:13s} {r[0]:5d} " + " ".join(f"{x:10d}" for x in r[1:]))
    tot = [sum(r[i] for r in rows.values()) for i in range(1 + len(cols))]
    print(f"{'total':13s} {tot[0]:5d} " + " ".join(f"{x:10d}" for x in tot[1:]))
    assert all(r[3] == 0 for r in rows.values())


def test_the_lse_bound_next_to_the_old_bar():
    """The derived LSE bound against the earlier bar (1e-4; the forms: 1e-4 * max(1, |lse|)) per case: printed; where it is looser (a large T: the peaked rows, steep slopes, saturated scores) the
    GPU test asserts both."""
    looser = []
    for c in R.CASES:
        t, parts, ref = _reference(c["id"], c["dtype"])
        worst, tmax = 0.0, 0.0
        for key in parts:
            _, lse, _, T, bound = ref[key]
            fin = torch.isfinite(lse)
            if fin.any():
                worst = max(worst, (bound[fin] / R.old_lse_bar(lse[fin], R.has_form(c))).max().item())
                tmax = max(tmax, T[fin].max().item())
        print(f"{c['id']}: the LSE bound is at most {worst:.3f} of the old bar (largest T {tmax:.1f})")
        if worst > 1.0:
            looser.append((c["id"], worst))
        assert math.isfinite(worst) and worst > 0
    print("looser than the old bar: " + ("; ".join(f"{i} {w:.2f}x" for i, w in looser) or "none"))
