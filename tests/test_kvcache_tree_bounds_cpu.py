"""CPU proof that the per-element bounds of tests/kvcache_ref.py are the right size for every case tests/test_kvcache_tree_gpu.py runs with a tree mask:
  1. the correct algorithm fits: kvcache_ref's emulations on the tree problem stay inside the out bound and the LSE bound (ratio <= 1), in both dtypes, on every
     listed case and on 36 seeded draws;
  2. they bite: every tree mutant a case names (kvcache_tree_ref.TMUTANTS: the fp64 result of a wrong rule 3 — a bit, a row or a base off by one, the word of the
     packed row, an unclamped or unreduced base, the second tile or the high dword left out, the 64th key on masked or wrapped) misses a bound by at least 10x, the
     factor tests/test_kvcache_bounds_cpu.py uses; every mutant is named by some case, and the tree keys carry the weight that makes it so;
  3. all-ones words ARE kvcache_ref.reference;
  4. the list covers what it must, and stays small.
No GPU, no kernel: fp64 (and one fp32 emulation) on the host.
"""
import functools

import pytest
import torch

import kvcache_ref as K
import kvcache_tree_ref as T

IDS = [c["id"] for c in T.CASES]
SWEEP = [f"tsweep{s}" for s in range(T.SWEEP)]
BITE = 10.0


@functools.lru_cache(maxsize=None)
def _reference(case_id, dtype):
    """(tensors, fp64 reference per sequence) of a case in `dtype`: computed once, shared by the tests below."""
    t = T.build(T.case_of(case_id), dtype)
    return t, T.reference(t)


# ---- 1. the correct algorithm fits --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case_id", IDS + SWEEP)
def test_emulation_fits(case_id, dtype):
    t, ref = _reference(case_id, dtype)
    c = t["case"]
    wo = wl = 0.0
    for b, (out, lse, A, Tm, n) in ref.items():
        wo = max(wo, K.out_ratio(T.emulate16(t, b), out, A, dtype))
        wl = max(wl, K.lse_ratio(T.emulate_lse32(t, b), lse, Tm, n, c["D"], K.lse_splits(c)))
    print(f"{case_id}: emulate16 at {wo:.3f} of the out bound, the fp32 LSE at {wl:.3f} of the LSE bound")
    assert wo <= 1.0 and wl <= 1.0


def test_the_emulations_leave_kvcache_ref_as_it_was():
    t, _ = _reference(IDS[0], T.BY_ID[IDS[0]]["dtype"])
    T.emulate16(t, 0), T.emulate_lse32(t, 0)
    assert K.seq_problem is T._seq_problem and K.hot_keys is T._hot_keys


# ---- 2. the bounds bite --------------------------------------------------------------------------------------------------------------------------------
def test_every_mutant_is_named():
    for c in T.CASES:
        assert set(c["tmutants"]) | {m for m, _ in c["tna"]} == set(T.TMUTANTS) and not set(c["tmutants"]) & {m for m, _ in c["tna"]}, c["id"]
        assert all(why for _, why in c["tna"]), c["id"]
    named = {m for c in T.CASES for m in c["tmutants"]}
    assert named == set(T.TMUTANTS), f"no case can have {set(T.TMUTANTS) - named}"


def _mutant_ratios(case_id, mutant, dtype):
    t, ref = _reference(case_id, dtype)
    c = t["case"]
    wo = wl = 0.0
    for b, (out, lse, A, Tm, n) in ref.items():
        mo, ml = T.attend_mut(t, b, mutant)
        wo = max(wo, K.out_ratio(mo, out, A, dtype))
        wl = max(wl, K.lse_ratio(ml, lse, Tm, n, c["D"], K.lse_splits(c)))
    return wo, wl


@pytest.mark.parametrize("case_id,mutant", [(c["id"], m) for c in T.CASES if not c["sched"] for m in c["tmutants"]])
def test_tree_mutant_misses_a_bound(case_id, mutant):
    wo, wl = _mutant_ratios(case_id, mutant, T.BY_ID[case_id]["dtype"])
    print(f"{case_id} / {mutant}: misses the out bound by {wo:.1f}x, the LSE bound by {wl:.1f}x")
    assert max(wo, wl) >= BITE, f"{case_id}: mutant {mutant} is only {wo:.2f}x / {wl:.2f}x outside the bounds — the case's inputs do not tell it from the definition"


@pytest.mark.parametrize("seed", range(T.SWEEP))
def test_a_tree_mutant_misses_a_bound_on_every_draw(seed):
    c = T.sweep_case(seed)
    got = {m: max(_mutant_ratios(c["id"], m, c["dtype"])) for m in c["tmutants"]}
    print(f"{c['id']} {c['mask']}: " + "  ".join(f"{m} {r:.1f}x" for m, r in got.items()))
    if c["tmutants"]:                                      # (a draw whose every sequence is empty has nothing for a tree mutant to act on)
        assert max(got.values()) >= BITE, f"{c}: no tree mutant is 10x outside the bounds"


# ---- 3. all-ones words are no mask -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", ["t4d-fp16-d64-g2-nq40-page64-s2", "tvq-bf16-d64-g4-tree", "t4d-fp8-bf16-d48-g2-nq5", "t4d-append-fp16-d104-g1-nq5"])
def test_all_ones_words_are_the_plain_definition(case_id):
    t = T.build(dict(T.BY_ID[case_id], mask="ones"))
    assert bool((t["words"] == -1).all())
    plain, tree = K.reference(t), T.reference(t)
    assert set(plain) == set(tree)
    for b in plain:
        for x, y in zip(plain[b][:4], tree[b][:4]):
            assert torch.equal(x, y), (case_id, b)


# ---- 4. the list itself, and the masks -----------------------------------------------------------------------------------------------------------------
def test_the_case_list_covers_the_minimum():
    cs = T.CASES
    G = lambda c: c["H"] // c["Hk"]                      # noqa: E731
    rows = lambda c: [nq for _, nq in K.rows_of(c)[0]]   # noqa: E731
    seqs = [(c, n, nq) for c in cs for n, nq in zip(c["lens"], rows(c)) if nq]
    assert all(c["causal"] for c in cs)
    for c in cs:
        assert c["B"] <= 5 and c["H"] <= 8 and c["cap"] <= 1024, c["id"]
    d4 = [c for c in cs if c["form"] == "4d"]
    assert {c["Nq"] for c in d4} >= {1, 5, 33, 40, 64} and all(c["Nq"] <= 64 for c in d4)
    assert {(n - nq) % 64 for c, n, nq in seqs if n >= nq} >= {0, 1, 40, 63}
    assert any((n - nq) // 64 != (n - 1) // 64 for c, n, nq in seqs if n >= nq and nq <= 64), "the new keys across a tile seam"
    assert any(0 <= n - nq < 64 for c, n, nq in seqs) and any(0 < n < nq for c, n, nq in seqs) and any(n == 0 for c, n, nq in seqs)
    assert any(c["cap"] in c["lens"] for c in cs)
    assert {c["splits"] for c in cs} >= {0, 1, 2, 3}
    assert any(c["splits"] > 1 and any(n - nq < lo < n for lo, hi in K._chunks(n, c["splits"])[1:]) for c, n, nq in seqs), "a chunk seam inside the new keys"
    assert {G(c) for c in cs} >= {1, 2, 4, 8} and any(c["Hk"] == 1 and G(c) > 1 for c in cs)
    assert {c["pack"] for c in cs} == {None, True, False}
    assert any(c["pack"] is True and c["form"] == "4d" and c["Nq"] * G(c) > 128 for c in cs), "two query blocks of packed rows"
    assert {c["page"] for c in cs} >= {0, 64, 128, 256}
    assert any(c["fp8"] and c["page"] for c in cs) and any(c["fp8"] and not c["page"] for c in cs)
    assert {c["D"] for c in cs if not c["fp8"]} >= {40, 64, 104, 128} and {c["D"] for c in cs if c["fp8"]} >= {48, 64, 112, 128}
    assert {c["dtype"] for c in cs} == {K.BF16, K.FP16}
    assert any(c["append"] == "4d" for c in cs) and any(c["append"] == "varlen" for c in cs)
    pk = [c for c in cs if c["form"] == "packed"]
    assert pk and all(c["lq"] == [300, 1, 130, 0, 64] for c in pk) and {c["max_q"] for c in pk} >= {300, 128}
    assert any(c["long_clear"] for c in pk) and any(not c["long_clear"] for c in pk)
    assert sum(1 for c in cs if c["sched"]) >= 2
    assert {c["mask"] for c in cs} >= {"tree", "pattern"}


def test_the_masks_are_what_the_list_says():
    own_clear = zero_at_base0 = long_ones = long_clear = 0
    for c in T.CASES:
        rows, asked = K.rows_of(c)
        for b, ws in enumerate(T.words_of(c)):
            assert len(ws) == asked[b]
            for t, w in enumerate(ws):
                assert -(1 << 63) <= w < (1 << 63)
                u = w & ((1 << 64) - 1)
                if t < 64:
                    assert u >> (t + 1) == 0, "sub-causal: no bit above the row's own"
                    own_clear += not u >> t & 1
                else:
                    long_ones += w == -1
                    long_clear += w != -1
                if c["mask"] == "tree" and 0 < t < 64:
                    anc = u & ~(1 << t)
                    assert u >> t & 1 and (anc == 0 or anc in [x & ((1 << 64) - 1) for x in ws[:t]]), "a tree row is its parent's word and its own bit"
            if ws and ws[0] == 0 and c["lens"][b] == rows[b][1]:
                zero_at_base0 += 1
    assert own_clear and zero_at_base0 and long_ones and long_clear


def test_bool_and_int64_forms_agree():
    g = torch.Generator().manual_seed(3)
    m = torch.rand(3, 64, 64, generator=g) < 0.5
    w = T.pack_bool(m)
    assert w.dtype == torch.int64 and torch.equal(T.bool_of(w, 64), m)
    assert int(T.pack_bool(torch.eye(64, dtype=torch.bool))[63]) == -(1 << 63)
    assert torch.equal(T.pack_bool(torch.ones(5, 5, dtype=torch.bool).tril()), torch.tensor([1, 3, 7, 15, 31]))


def test_tree_keys_carry_weight():
    """A masked earlier sibling and a visible ancestor of the last row hold a visible share of the rows that can see them: at least 2 % of the probability of some
    head's row under the plain causal rule, on every sequence that has such keys."""
    for c in T.CASES:
        if c["sched"]:
            continue
        t, ref = _reference(c["id"], c["dtype"])
        for b in ref:
            n, nq = t["lens"][b], t["rows"][b][1]
            keys = [j for j in T.tree_keys(c, b, n) if j >= max(n - nq, 0)]
            if not keys:
                continue
            P = torch.softmax(K.scores(K.seq_problem(t, b))[:, nq - 1], dim=-1).nan_to_num(0.0)      # (H, n): the last row sees every key
            assert max(P[:, j].max().item() for j in keys) >= 0.02, (c["id"], b)
