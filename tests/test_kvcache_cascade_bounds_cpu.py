"""CPU proof that the bounds of tests/kvcache_cascade_ref.py are the right size for every case tests/test_kvcache_cascade_gpu.py runs:
  1. the correct algorithm fits: the emulation of what runs — per-level chunks, fp32 partials, the skipping merge over ns0 + ns1 parts, one rounding — stays inside
     the out bound and the LSE bound on every listed case and on seeded draws;
  2. they bite: every mutant a case names (kvcache_cascade_ref.MUTANTS, each the fp64 result of ONE wrong statement) misses a bound by at least 10x, the project's
     factor; every mutant is named by some case;
  3. the definition IS kvcache_ref.reference on the equivalent flat problem — the shared pages prepended to each sequence's table — wherever plen_g is a page multiple;
  4. the list covers what the GPU test must run.
No GPU, no kernel: fp64 (and one fp32 emulation) on the host.
"""
import functools
import math

import pytest
import torch

import kvcache_cascade_ref as CR
import kvcache_ref as K

IDS = [c["id"] for c in CR.CASES]
SWEEP = 12
BITE = 10.0


@functools.lru_cache(maxsize=None)
def _reference(case_id):
    t = CR.build(CR.case_of(case_id))
    return t, CR.reference(t)


# ---- 1. the correct algorithm fits ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", IDS + [f"sweep{s}" for s in range(SWEEP)])
def test_emulation_fits(case_id):
    t, ref = _reference(case_id)
    out, lse = CR.emulate(t)
    wo, wl = CR.ratios(t, out, lse, ref)
    print(f"{case_id}: the emulated out at {wo:.3f} of its bound, the fp32 LSE at {wl:.3f} of the LSE bound ({sum(CR.chunks_of(t))} parts)")
    assert wo <= 1.0 and wl <= 1.0
    unseen = torch.isposinf(ref[1])
    assert bool((out.transpose(0, 1)[unseen] == 0).all())


def test_the_emulations_merge_skips_what_tfa_merge_would_scale():
    """The emulated merge on parts whose dead O words are NaN: the result is the one with zeros there (a skip), where weighting by 0 gives NaN."""
    lses = torch.tensor([[1.0], [-math.inf]], dtype=torch.float64)
    o = torch.tensor([[2.0], [math.nan]], dtype=torch.float64)
    live = torch.isfinite(lses)
    w = torch.where(live, torch.exp(lses - 1.0), torch.zeros_like(lses))
    assert bool(torch.isnan((w * o).sum(0)).all()) and torch.where(live, w * o, torch.zeros(1, dtype=torch.float64)).sum(0).item() == 2.0


# ---- 2. the bounds bite -----------------------------------------------------------------------------------------------------------------------------------------
def test_every_mutant_is_named():
    for c in CR.CASES:
        assert set(c["mutants"]) | {m for m, _ in c["na"]} == set(CR.MUTANTS) and not set(c["mutants"]) & {m for m, _ in c["na"]}, c["id"]
        assert all(why for _, why in c["na"]), c["id"]
        assert c["mutants"], c["id"]
    named = {m for c in CR.CASES for m in c["mutants"]}
    assert named == set(CR.MUTANTS), f"no case can have {set(CR.MUTANTS) - named}"


@pytest.mark.parametrize("case_id,mutant", [(c["id"], m) for c in CR.CASES if not c["sched"] for m in c["mutants"]])
def test_mutant_misses_a_bound(case_id, mutant):
    t, ref = _reference(case_id)
    mo, ml = CR.reference(t, mutant)[:2]
    wo, wl = CR.ratios(t, mo, ml, ref)
    print(f"{case_id} / {mutant}: misses the out bound by {wo:.1f}x, the LSE bound by {wl:.1f}x")
    assert max(wo, wl) >= BITE, f"{case_id}: mutant {mutant} is only {wo:.2f}x / {wl:.2f}x outside the bounds — the case's inputs do not tell it from the definition"


# ---- 3. the definition is the flat call's ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", IDS[:6] + ["cs-bf16-d64-noncausal-s32"])
def test_definition_is_kvcache_refs_on_the_flat_problem(case_id):
    t, (out, lse, A, T, _) = _reference(case_id)
    ft, same = CR.flat(t)
    plain = K.reference(ft)
    checked = 0
    for b, (o, l, a, tm, _) in plain.items():
        if not same[b]:
            continue
        q0, nq = ft["rows"][b]
        for x, y in ((o, out[q0:q0 + nq]), (l, lse[:, q0:q0 + nq]), (a, A[q0:q0 + nq]), (tm, T[:, q0:q0 + nq])):
            assert torch.allclose(x, y, rtol=1e-12, atol=1e-12) and torch.equal(torch.isposinf(x), torch.isposinf(y)), (case_id, b)
        checked += 1
    assert checked >= 2, case_id


# ---- 4. the list itself -----------------------------------------------------------------------------------------------------------------------------------------
def test_the_case_list_covers_what_the_gpu_test_must_run():
    cs = CR.CASES
    assert {(c["dtype"], c["D"]) for c in cs} >= {(CR.BF16, 64), (CR.BF16, 128), (CR.FP16, 64), (CR.FP16, 128)}
    assert {(c["H"], c["Hk"]) for c in cs} >= {(8, 2), (4, 4)} and {c["pack"] for c in cs} == {None, True, False}
    assert {c["splits"] for c in cs} >= {(1, 1), (3, 1), (1, 2), (3, 2)}
    assert {p for c in cs for _, p in c["groups"]} >= {0, 1, 64, 130}
    assert {u for c in cs for _, u in c["seqs"]} >= {0, 1, 63, 64, 65, 129} and {n for c in cs for n, _ in c["seqs"]} >= {0, 1, 5, 33}
    assert all(c["tail"] >= 1 for c in cs) and all(len(c["seqs"]) > sum(n for n, _ in c["groups"]) for c in cs)       # a row in no sequence, a sequence in no group
    assert all([n for n, _ in c["groups"]] == [3, 1, 2] for c in cs)
    wide = [c for c in cs if max(r1 - r0 for r0, r1 in CR.layout(c)[1]) * (c["H"] // c["Hk"]) > 128 and c["pack"] is not False]
    assert wide, "no group whose packed rows span two query blocks"
    assert any(c["sched"] for c in cs) and any(not c["causal"] for c in cs)
    assert len(cs) <= 20
