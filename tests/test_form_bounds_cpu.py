"""CPU proof that the per-element backward bound of tests/form_ref.py is the right size for every case tests/test_forms_bwd_bounds_gpu.py runs:
  1. without a form it IS oracle.attn_bwd_bounds / attn_bwd_reference (1e-12 relative; GQA, Nq < Nk, Nq > Nk) — the bound with kv_p16=False; the one derived
     term the default adds (the dK/dV launch's second 16-bit rounding, form_ref.bwd_bounds) touches Ak alone and at most doubles it;
  2. the correct algorithm fits: form_ref.emulate16 (the kernels' 16-bit rounding points, fp64 elsewhere) stays inside eps16 * A + 1e-6 for all three
     gradients, in both dtypes, on every case of the GPU list and every draw of its seeded sweep;
  3. it bites: for every mutant a case names (form_ref.MUTANTS: a window edge moved by one key, the ALiBi distance without Nk - Nq, batch 0's slopes for every
     batch entry, 1 - tanh^2 omitted, the cap 2 % off, the bias read one row off or by the K/V head, the next sequence's first key visible), the mutant's fp64
     gradients miss the bound by at least 10x in some element.  A condition on the cases' inputs, not on the kernels.  Every case names at least one mutant;
     a mutant a case cannot have for a structural reason is listed in its `na` with the reason (form_ref._cases).
No GPU, no kernel: fp64 on the host.
"""
import functools

import pytest
import torch

import form_ref as F

IDS = [c["id"] for c in F.CASES]
BITE = 10.0


def _parts(t):
    """A case as a list of (q, k, v, dout, form, k_next, v_next) in (1|B, H, n, D) form: itself, or its sequences."""
    if t["case"]["kind"] == "varlen":
        return [(q, k, v, do, f, kn, vn) for _, q, k, v, do, f, kn, vn in F.sequences(t)]
    return [(t["q"], t["k"], t["v"], t["dout"], t["form"], None, None)]


@functools.lru_cache(maxsize=None)
def _reference(case_id, dtype):
    """(parts, [(ref grads, bounds, emulated grads)] per part) of a case in `dtype`: computed once, shared by the tests below."""
    case = F.BY_ID[case_id] if case_id in F.BY_ID else F.sweep_case(int(case_id[len("sweep"):]))
    t = F.build(case, dtype)
    parts, res = _parts(t), []
    for q, k, v, do, f, _, _ in parts:
        if k.shape[2] == 0:
            res.append(None)
            continue
        emu, o16 = F.emulate16(q, k, v, do, t["sc"], dtype, **f)
        res.append((F.ref_grads(q, k, v, do, t["sc"], **f), F.bwd_bounds(q, k, v, o16, do, t["sc"], **f), emu))
    return t, parts, res


# ---- 1. no form: the existing oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("B,H,Hk,Nq,Nk,D", [(2, 4, 2, 96, 96, 64), (1, 4, 1, 70, 203, 40), (1, 2, 2, 257, 130, 128), (2, 3, 3, 33, 65, 72)])
def test_no_form_is_the_existing_oracle(oracle, causal, B, H, Hk, Nq, Nk, D):
    dtype, sc = torch.bfloat16, 0.11
    q, k, v = F.rnd((B, H, Nq, D), dtype, 1), F.rnd((B, Hk, Nk, D), dtype, 2), F.rnd((B, Hk, Nk, D), dtype, 3)
    dout = F.rnd((B, H, Nq, D), dtype, 4)
    window = (-1, 0) if causal else (-1, -1)
    out16 = F.ref_fwd(q, k, v, sc, window=window)[0].float().to(dtype)
    theirs = oracle.attn_bwd_bounds(q, k, v, out16, dout, causal, sc)
    for mine, them in ((F.ref_grads(q, k, v, dout, sc, window=window), oracle.attn_bwd_reference(q, k, v, dout, causal, sc)),
                       (F.bwd_bounds(q, k, v, out16, dout, sc, kv_p16=False, window=window), theirs)):
        for a, b in zip(mine, them):
            assert a.shape == b.shape
            assert (a - b).abs().max().item() <= 1e-12 * b.abs().max().item()
    # the dK/dV launch's second rounding (kv_p16, the default) touches Ak alone, and at most doubles it
    aq, ak, av = F.bwd_bounds(q, k, v, out16, dout, sc, window=window)
    assert (aq - theirs[0]).abs().max().item() <= 1e-12 * theirs[0].abs().max().item() and (av - theirs[2]).abs().max().item() <= 1e-12 * theirs[2].abs().max().item()
    assert bool((ak >= theirs[1] * (1 - 1e-12)).all()) and bool((ak <= 2 * theirs[1] * (1 + 1e-12)).all())
    lse = F.ref_fwd(q, k, v, sc, window=window)[1]
    assert bool(torch.isposinf(lse).any()) == (causal and Nq > Nk), "rows above the bottom-right diagonal see nothing"


# ---- 2. the correct algorithm fits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case_id", IDS + [f"sweep{s}" for s in range(48)])
def test_emulation_fits(case_id, dtype):
    t, parts, res = _reference(case_id, dtype)
    worst = 0.0
    for r in res:
        if r is None:
            continue
        ref, bounds, emu = r
        worst = max([worst] + F.ratios(emu, ref, bounds, dtype))
    print(f"{case_id}: emulate16 at {worst:.3f} of the bound")
    assert worst <= 1.0


def test_the_case_list_covers_the_minimum():
    """What the GPU file must cover, asserted on the list itself so that it cannot shrink unnoticed."""
    fx = [c for c in F.CASES if c["kind"] == "fixed"]
    vl = [c for c in F.CASES if c["kind"] == "varlen"]
    assert all(c.get("Nq", 0) <= 450 and c.get("Nk", 0) <= 450 and c["B"] <= 2 and c["H"] <= 4 for c in fx) and all(max(c["lq"] + c["lk"]) <= 450 for c in vl)
    plain = lambda c: c["slopes"] is None and not c["cap"] and c["bias"] is None   # noqa: E731
    win = [c for c in fx if plain(c)]
    for w in [(0, 0), (63, 0), (64, 0), (65, 0), (37, 20), (128, 128), (-1, 64), (64, -1)]:
        assert {(c["Nq"], c["Nk"]) for c in win if c["window"] == w and not c["causal"]} == set(F.SHAPES), w
    assert {(c["Nq"], c["Nk"]) for c in win if c["causal"] and c["window"] == (200, 77)} == set(F.SHAPES)
    assert {c["dtype"] for c in win} == {F.BF16, F.FP16} and {c["D"] for c in win} == {40, 64, 96, 128} and {c["H"] // c["Hk"] for c in win} == {1, 2, 4}
    al = [c for c in fx if c["slopes"] is not None and not c["cap"]]
    assert {c["slopes"] for c in al} == {"H", "BH", "steep", "zeroneg"} and all(c["B"] == 2 for c in al if c["slopes"] == "BH")
    assert {"full", "causal", "window"} <= {"causal" if c["causal"] else "full" if c["window"] == (-1, -1) else "window" for c in al}
    assert any(c["Nq"] < c["Nk"] for c in al) and any(c["Nq"] > c["Nk"] for c in al)
    cp = [c for c in fx if c["cap"]]
    assert {(5.0, 2.0), (5.0, 8.0), (50.0, 0.5)} <= {(c["cap"], c["std"]) for c in cp}
    assert any(c["slopes"] for c in cp) and any(not c["slopes"] for c in cp) and any(F.eff_window(c["causal"], c["window"])[0] >= 0 for c in cp)
    bi = [c for c in fx if c["bias"] is not None]
    assert {c["bias"]["shape"] for c in bi} == {(True, True), (False, True), (True, False), (False, False)} and {c["bias"]["f32"] for c in bi} == {False, True}
    assert {c["bias"]["layout"] for c in bi} == {"contig", "padded", "odd", "expanded"} and any(c["bias"]["masked"] for c in bi)
    assert any(c["causal"] for c in bi) and any(c["window"] != (-1, -1) and not c["causal"] for c in bi) and any(c["H"] > c["Hk"] for c in bi)
    assert all(c["lq"] == [300, 1, 257, 0, 64] and c["lk"] == [300, 90, 200, 7, 64] for c in vl)
    kinds = {(F.eff_window(c["causal"], c["window"]) != (-1, -1), c["slopes"] is not None, bool(c["cap"])) for c in vl}
    assert {(True, False, False), (False, False, True), (True, True, True)} <= kinds and any(k[1] and not k[2] for k in kinds)
    assert len(F.AUTOGRAD_IDS) >= 6


# ---- 3. the bound bites -----------------------------------------------------------------------------------------------------------------------
def test_every_case_names_a_mutant():
    for c in F.CASES:
        assert c["mutants"], c["id"]
        assert all(m in F.MUTANTS for m in c["mutants"]) and all(m in F.MUTANTS and why for m, why in c["na"]), c["id"]
        forms = {"wl+1": "window", "wr+1": "window", "alibi_shift0": "alibi", "slopes_b0": "alibi", "no_dtanh": "cap", "cap*1.02": "cap", "bias_row": "bias",
                 "bias_kvhead": "bias", "next_key": "varlen"}
        for form in set(forms.values()):                 # at most one mutant per form not applicable — but both of the cap's in the near-linear regime
            n = sum(1 for m, _ in c["na"] if forms[m] == form)
            assert n <= (2 if form == "cap" and c["cap"] >= 50 else 1), f"{c['id']}: {n} mutants of {form} not applicable"
        assert not set(c["mutants"]) & {m for m, _ in c["na"]}, c["id"]


def _mutant_ratio(case_id, mutant, dtype):
    t, parts, res = _reference(case_id, dtype)
    G = t["case"]["H"] // t["case"]["Hk"]
    worst = 0.0
    batch_form = F.mutant_form(t["form"], mutant, G) if mutant == "slopes_b0" else None      # (mutated over the batch, then taken per sequence)
    seqs = [b for b, *_ in F.sequences(t)] if t["case"]["kind"] == "varlen" else [None]
    for b, (q, k, v, do, f, kn, vn), r in zip(seqs, parts, res):
        if r is None:
            continue
        ref, bounds, _ = r
        if batch_form is not None:
            mg = F.ref_grads(q, k, v, do, t["sc"], **(F.seq_form(batch_form, b) if b is not None else batch_form))
        else:
            mg = F.mutant_grads(mutant, q, k, v, do, t["sc"], f, kn, vn)
        worst = max([worst] + F.ratios(mg, ref, bounds, dtype))
    return worst


@pytest.mark.parametrize("case_id,mutant", [(c["id"], m) for c in F.CASES for m in c["mutants"]])
def test_mutant_misses_the_bound(case_id, mutant):
    worst = _mutant_ratio(case_id, mutant, F.BY_ID[case_id]["dtype"])
    print(f"{case_id} / {mutant}: misses eps16 * A + 1e-6 by {worst:.1f}x")
    assert worst >= BITE, f"{case_id}: mutant {mutant} is only {worst:.2f}x outside the bound — the case's inputs do not tell it from the correct backward"


@pytest.mark.parametrize("seed", range(48))
def test_a_mutant_misses_the_bound_on_every_draw(seed):
    """The seeded sweep's draws name no mutants: at least one of those their forms could have must miss the bound by 10x."""
    c = F.sweep_case(seed)
    got = {m: _mutant_ratio(c["id"], m, c["dtype"]) for m in F.candidate_mutants(c)}
    print(f"{c['id']}: " + "  ".join(f"{m} {r:.1f}x" for m, r in got.items()))
    assert got and max(got.values()) >= BITE, f"{c}: no mutant is 10x outside the bound"
