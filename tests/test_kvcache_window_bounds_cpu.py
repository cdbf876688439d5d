"""CPU proof that the per-element bounds of tests/kvcache_window_ref.py are the right size for every case tests/test_kvcache_window_gpu.py runs:
  1. the correct algorithm fits: the emulations over the windowed chunks stay inside the out bound and the LSE bound (ratio <= 1), in both dtypes, on every
     listed case and on 24 seeded draws;
  2. they bite: every window mutant a case names (kvcache_window_ref.WMUTANTS: the fp64 result of a wrong window — an edge off by one key, rounded to a tile, taken
     from the wrong row, position or row count, a dropped chunk seam) misses a bound by at least 10x, the factor tests/test_kvcache_bounds_cpu.py uses; every
     mutant is named by some case, and the window-edge keys carry the weight that makes it so;
  3. with w - 1 >= the capacity the windowed definition IS kvcache_ref.reference;
  4. the list covers what it must, and stays small.
No GPU, no kernel: fp64 (and one fp32 emulation) on the host.
"""
import functools

import pytest
import torch

import kvcache_ref as K
import kvcache_window_ref as W

IDS = [c["id"] for c in W.CASES]
SWEEP = [f"wsweep{s}" for s in range(W.SWEEP)]
BITE = 10.0


@functools.lru_cache(maxsize=None)
def _reference(case_id, dtype):
    """(tensors, fp64 reference per sequence) of a case in `dtype`: computed once, shared by the tests below."""
    t = W.build(W.case_of(case_id), dtype)
    return t, W.reference(t)


# ---- 1. the correct algorithm fits --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case_id", IDS + SWEEP)
def test_emulation_fits(case_id, dtype):
    t, ref = _reference(case_id, dtype)
    c = t["case"]
    wo = wl = 0.0
    for b, (out, lse, A, T, n) in ref.items():
        wo = max(wo, K.out_ratio(W.emulate16(t, b), out, A, dtype))
        wl = max(wl, K.lse_ratio(W.emulate_lse32(t, b), lse, T, n, c["D"], K.lse_splits(c)))
    print(f"{case_id}: emulate16 at {wo:.3f} of the out bound, the fp32 LSE at {wl:.3f} of the LSE bound")
    assert wo <= 1.0 and wl <= 1.0


# ---- 2. the bounds bite --------------------------------------------------------------------------------------------------------------------------------
def test_every_mutant_is_named():
    for c in W.CASES:
        assert c["wmutants"], c["id"]
        assert set(c["wmutants"]) | {m for m, _ in c["wna"]} == set(W.WMUTANTS) and not set(c["wmutants"]) & {m for m, _ in c["wna"]}, c["id"]
        assert all(why for _, why in c["wna"]), c["id"]
    named = {m for c in W.CASES for m in c["wmutants"]}
    assert named == set(W.WMUTANTS), f"no case can have {set(W.WMUTANTS) - named}"


def _mutant_ratios(case_id, mutant, dtype):
    t, ref = _reference(case_id, dtype)
    c = t["case"]
    wo = wl = 0.0
    for b, (out, lse, A, T, n) in ref.items():
        mo, ml = W.attend_mut(t, b, mutant)
        wo = max(wo, K.out_ratio(mo, out, A, dtype))
        wl = max(wl, K.lse_ratio(ml, lse, T, n, c["D"], K.lse_splits(c)))
    return wo, wl


@pytest.mark.parametrize("case_id,mutant", [(c["id"], m) for c in W.CASES for m in c["wmutants"]])
def test_window_mutant_misses_a_bound(case_id, mutant):
    wo, wl = _mutant_ratios(case_id, mutant, W.BY_ID[case_id]["dtype"])
    print(f"{case_id} / {mutant}: misses the out bound by {wo:.1f}x, the LSE bound by {wl:.1f}x")
    assert max(wo, wl) >= BITE, f"{case_id}: mutant {mutant} is only {wo:.2f}x / {wl:.2f}x outside the bounds — the case's inputs do not tell it from the definition"


@pytest.mark.parametrize("seed", range(W.SWEEP))
def test_a_window_mutant_misses_a_bound_on_every_draw(seed):
    c = W.sweep_case(seed)
    got = {m: max(_mutant_ratios(c["id"], m, c["dtype"])) for m in c["wmutants"]}
    print(f"{c['id']} w={c['w']}: " + "  ".join(f"{m} {r:.1f}x" for m, r in got.items()))
    if c["wmutants"]:                                      # (a draw whose every window starts in front of key 0 has nothing for a window mutant to act on)
        assert max(got.values()) >= BITE, f"{c}: no window mutant is 10x outside the bounds"


# ---- 3. a window that reaches every key is no window ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", ["w4d-fp16-d64-g2-nq5-w2-page64-s2", "wvq-bf16-d64-g4-w128", "w4d-fp8-fp16-d128-mqa-nq5-w2"])
def test_full_window_is_the_plain_definition(case_id):
    c = dict(W.BY_ID[case_id])
    for w in (c["cap"] + 1, c["cap"] + 1000):              # w - 1 >= cap
        c["w"] = w
        t = K.build(c)
        plain, win = K.reference(t), W.reference(t)
        assert set(plain) == set(win)
        for b in plain:
            for x, y in zip(plain[b][:4], win[b][:4]):
                assert torch.equal(x, y), (case_id, b)


# ---- 4. the list itself ------------------------------------------------------------------------------------------------------------------------------
def test_the_case_list_covers_the_minimum():
    cs = W.CASES
    G = lambda c: c["H"] // c["Hk"]                      # noqa: E731
    assert all(c["causal"] for c in cs)
    assert {c["w"] for c in cs} >= {1, 2, 64, 65, 100, 128, 512}
    d4 = [c for c in cs if c["form"] == "4d"]
    assert {c["Nq"] for c in d4} >= {1, 5, 33, 130}
    pk = [c for c in cs if c["form"] == "packed"]
    assert pk and all(c["lq"] == [300, 1, 130, 0, 64] for c in pk) and {c["max_q"] for c in pk} >= {300, 128}
    for c in cs:
        assert c["B"] <= 5 and c["H"] <= 8 and c["cap"] <= 1024, c["id"]
        assert all(n in K.LENGTHS or n == c["cap"] for n in c["lens"]), c["id"]
    rows = lambda c: [nq for _, nq in K.rows_of(c)[0]]   # noqa: E731
    assert any(any(nq and n < nq for n, nq in zip(c["lens"], rows(c))) for c in cs), "len_b < nq_b"
    assert any(any(nq and 1 <= n <= c["w"] for n, nq in zip(c["lens"], rows(c))) for c in cs), "len_b <= w"
    assert any(c["cap"] in c["lens"] for c in cs)
    assert {c["page"] for c in cs} >= {0, 64, 128, 256}
    assert {c["splits"] for c in cs} >= {0, 1, 2, 3, 4}
    assert any(c["splits"] > 1 and any(lo >= hi for n, nq in zip(c["lens"], rows(c)) if nq and n
                                       for lo, hi in W.win_chunks(n, nq, c["w"] - 1, c["splits"])[1:]) for c in cs), "trailing chunks empty"
    assert {G(c) for c in cs} >= {1, 2, 4, 8} and any(c["Hk"] == 1 and G(c) > 1 for c in cs)
    assert {c["pack"] for c in cs} == {None, True, False}
    assert any(c["fp8"] and c["page"] for c in cs) and any(c["fp8"] and not c["page"] for c in cs)
    assert sum(1 for c in cs if c["sched"]) >= 2
    assert any(c["append"] == "4d" for c in cs)
    assert {c["D"] for c in cs if not c["fp8"]} >= {40, 64, 104, 128} and {c["D"] for c in cs if c["fp8"]} >= {48, 64, 112, 128}
    assert {c["dtype"] for c in cs} == {K.BF16, K.FP16}


def test_edge_keys_carry_weight():
    """The window-edge keys of the first and last row hold a visible share of the rows that see them (the weight build() gives them): at least 2 % of the
    probability of some head's row, on every case that has such a key."""
    for c in W.CASES:
        t, ref = _reference(c["id"], c["dtype"])
        for b in ref:
            n, nq = t["lens"][b], t["rows"][b][1]
            inside = [j for j in (n - nq - (c["w"] - 1), n - 1 - (c["w"] - 1)) if 0 <= j < n]
            if not inside:
                continue
            p = W.win_problem(t, b)
            P = torch.softmax(K.scores(p)[:, [0, nq - 1]], dim=-1).nan_to_num(0.0)
            assert max(P[:, :, j].max().item() for j in inside) >= 0.02, (c["id"], b)
