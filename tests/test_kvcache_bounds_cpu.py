"""CPU proof that the per-element bounds of tests/kvcache_ref.py are the right size for every case tests/test_kvcache_fwd_bounds_gpu.py runs:
  1. with one chunk, a contiguous 16-bit cache and G = 1 the definition IS oracle.exact64 and A is oracle.abs_weighted — to 2^-23 relative, the floor the C
     oracle's fp32 output and fp32 softmax_scale set — and form_ref.ref_fwd (fp64 throughout) to 1e-12 relative;
  2. the correct algorithm fits: kvcache_ref.emulate16 (the kernels' rounding points — P rounded tile by tile against the running maximum, the chunks, the
     merge, v_descale in front of the one rounding of O; fp64 elsewhere) stays inside the out bound, and a tile-ordered fp32 emulation of the LSE inside the
     derived LSE bound, in both dtypes, on every case of the GPU list and every draw of its seeded sweep;
  3. they bite: every mutant a case names (kvcache_ref.MUTANTS: a length, the causal diagonal, a chunk seam, a page, a V tile, a head, a packed position, a
     descale, an unclamped row count, an unquantised append, each off by one step) misses the out bound or the LSE bound by at least 10x in some element.  A
     condition on the cases' inputs, not on the kernels.  Every mutant a case does not name is in its `na` with the reason;
  4. the list covers what it must, and stays small.
No GPU, no kernel: fp64 (and one fp32 emulation) on the host.
"""
import functools
import math

import pytest
import torch

import kvcache_ref as K

IDS = [c["id"] for c in K.CASES]
SWEEP = [f"sweep{s}" for s in range(48)]
BITE = 10.0


@functools.lru_cache(maxsize=None)
def _reference(case_id, dtype):
    """(tensors, fp64 reference per sequence) of a case in `dtype`: computed once, shared by the tests below."""
    t = K.build(K.case_of(case_id), dtype)
    return t, K.reference(t)


# ---- 1. the plain problem: the existing oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D,Nq,lens", [(64, 5, [65, 300]), (40, 1, [128, 1]), (128, 33, [129, 7])])
def test_plain_case_is_the_existing_oracle(oracle, causal, D, Nq, lens):
    c = K._case("plain", dtype=torch.bfloat16, D=D, H=3, Hk=3, Nq=Nq, lens=lens, cap=320, causal=causal, seed=77)
    t = K.build(c)
    for b, (out, lse, A, _, n) in K.reference(t).items():
        q0, nq = t["rows"][b]
        q = t["q"][q0:q0 + nq].transpose(0, 1).unsqueeze(0)
        k, v = (x[b, :n].transpose(0, 1).unsqueeze(0) for x in (t["k_cache"], t["v_cache"]))
        o64, l64 = oracle.exact64(q, k, v, causal, t["sc"], return_lse=True)
        a64 = oracle.abs_weighted(q, k, v, causal, t["sc"])
        seen = torch.isfinite(lse)
        assert bool(seen.all()) == (not causal or n >= nq)
        # (the C oracle returns fp32: its own rounding, 2^-24 relative, is the floor of this comparison)
        for mine, them in ((out, o64[0].transpose(0, 1)), (A, a64[0].transpose(0, 1))):
            assert (mine - them.double()).abs().max().item() <= 2.0 ** -23 * them.abs().max().item() + 1e-12
        assert (lse[seen] - l64[0].double()[seen]).abs().max().item() <= 2.0 ** -22 * max(1.0, l64[0][seen].abs().max().item())


def test_plain_case_in_fp64():
    """The same identity without the C oracle's fp32 output in the way: against form_ref.ref_fwd (fp64 throughout), to 1e-12 relative."""
    c = K._case("plain64", dtype=torch.float16, D=64, H=4, Hk=4, Nq=5, lens=[65, 300, 3], cap=320, causal=True, seed=78)
    t = K.build(c)
    for b, (out, lse, A, _, n) in K.reference(t).items():
        q0, nq = t["rows"][b]
        q = t["q"][q0:q0 + nq].transpose(0, 1).unsqueeze(0)
        k, v = (x[b, :n].transpose(0, 1).unsqueeze(0) for x in (t["k_cache"], t["v_cache"]))
        o, l, a = K.F.ref_fwd(q, k, v, t["sc"], window=(-1, 0))
        for mine, them in ((out, o[0].transpose(0, 1)), (A, a[0].transpose(0, 1))):
            assert (mine - them).abs().max().item() <= 1e-12 * max(them.abs().max().item(), 1e-30)
        assert torch.equal(torch.isposinf(lse), torch.isposinf(l[0]))
        fin = torch.isfinite(lse)
        assert (lse[fin] - l[0][fin]).abs().max().item() <= 1e-12 * l[0][fin].abs().max().item()


# ---- 2. the correct algorithm fits --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case_id", IDS + SWEEP)
def test_emulation_fits(case_id, dtype):
    t, ref = _reference(case_id, dtype)
    c = t["case"]
    wo = wl = 0.0
    for b, (out, lse, A, T, n) in ref.items():
        wo = max(wo, K.out_ratio(K.emulate16(t, b), out, A, dtype))
        wl = max(wl, K.lse_ratio(K.emulate_lse32(t, b), lse, T, n, c["D"], K.lse_splits(c)))
    print(f"{case_id}: emulate16 at {wo:.3f} of the out bound, the fp32 LSE at {wl:.3f} of the LSE bound")
    assert wo <= 1.0 and wl <= 1.0


# ---- 3. the bounds bite --------------------------------------------------------------------------------------------------------------------------------
def test_every_case_names_its_mutants():
    for c in K.CASES:
        assert c["mutants"], c["id"]
        assert set(c["mutants"]) | {m for m, _ in c["na"]} == set(K.MUTANTS) and not set(c["mutants"]) & {m for m, _ in c["na"]}, c["id"]
        assert all(why for _, why in c["na"]), c["id"]
    named = {m for c in K.CASES for m in c["mutants"]}
    assert named == set(K.MUTANTS), f"no case can have {set(K.MUTANTS) - named}"


def _mutant_ratios(case_id, mutant, dtype):
    t, ref = _reference(case_id, dtype)
    c = t["case"]
    wo = wl = 0.0
    for b, (out, lse, A, T, n) in ref.items():
        mo, ml = K.attend_mut(t, b, mutant)
        wo = max(wo, K.out_ratio(mo, out, A, dtype))
        wl = max(wl, K.lse_ratio(ml, lse, T, n, c["D"], K.lse_splits(c)))
    return wo, wl


@pytest.mark.parametrize("case_id,mutant", [(c["id"], m) for c in K.CASES for m in c["mutants"]])
def test_mutant_misses_a_bound(case_id, mutant):
    wo, wl = _mutant_ratios(case_id, mutant, K.BY_ID[case_id]["dtype"])
    print(f"{case_id} / {mutant}: misses the out bound by {wo:.1f}x, the LSE bound by {wl:.1f}x")
    assert max(wo, wl) >= BITE, f"{case_id}: mutant {mutant} is only {wo:.2f}x / {wl:.2f}x outside the bounds — the case's inputs do not tell it from the definition"


# which bound sees which defect, as the list is built: a wrong V or a wrong output scale cannot move the LSE, a wrong LSE scale cannot move out
OUT_ONLY, LSE_ONLY = {"v_tile", "vd_twice"}, {"kd_not_in_lse"}


@pytest.mark.parametrize("mutant", K.MUTANTS)
def test_which_bound_sees_the_mutant(mutant):
    got = [_mutant_ratios(c["id"], mutant, c["dtype"]) for c in K.CASES if mutant in c["mutants"] and not c["long"]][:4]
    assert got
    print(f"{mutant}: " + "  ".join(f"out {o:.1f}x lse {l:.1f}x" for o, l in got))
    if mutant in OUT_ONLY:
        assert all(l <= 1.0 and o >= BITE for o, l in got)
    elif mutant in LSE_ONLY:
        assert all(o <= 1.0 and l >= BITE for o, l in got)
    else:
        assert all(o >= BITE or l >= BITE for o, l in got)


@pytest.mark.parametrize("seed", range(48))
def test_a_mutant_misses_a_bound_on_every_draw(seed):
    c = K.sweep_case(seed)
    got = {m: max(_mutant_ratios(c["id"], m, c["dtype"])) for m in c["mutants"]}
    print(f"{c['id']}: " + "  ".join(f"{m} {r:.1f}x" for m, r in got.items()))
    assert got and max(got.values()) >= BITE, f"{c}: no mutant is 10x outside the bounds"


# ---- 4. the list itself ------------------------------------------------------------------------------------------------------------------------------
def test_the_case_list_covers_the_minimum():
    """What the GPU file must cover, asserted on the list itself so that it cannot shrink unnoticed — and the caps that keep it quick."""
    cs = K.CASES
    G = lambda c: c["H"] // c["Hk"]                      # noqa: E731
    long, auto = [c for c in cs if c["long"]], [c for c in cs if c["auto"]]
    assert {c["dtype"] for c in long} == {K.BF16, K.FP16} and all(c["lens"] == [5000] and c["Nq"] == 1 and c["splits"] == 8 for c in long) and len(long) == 2
    # the one case the issue asks for above the cap besides the two long ones: num_splits = 0 over a paged capacity >= 4096, lengths <= 700
    assert len(auto) == 1 and all(c["splits"] == 0 and c["cap"] >= 4096 and c["page"] and max(c["lens"]) <= 700 for c in auto)
    for c in cs:
        assert c["B"] <= 5 and c["H"] <= 8, c["id"]
        assert c["cap"] <= 1024 or c["long"] or c["auto"], c["id"]
        assert all(n in K.LENGTHS or n == c["cap"] for n in c["lens"]), c["id"]
    assert {c["dtype"] for c in cs} == {K.BF16, K.FP16}
    assert {c["D"] for c in cs if not c["fp8"]} >= {40, 64, 104, 128} and {c["D"] for c in cs if c["fp8"]} >= {48, 64, 112, 128}
    assert {G(c) for c in cs} >= {1, 2, 4, 8} and any(c["Hk"] == 1 and G(c) > 1 for c in cs)
    d4 = [c for c in cs if c["form"] == "4d"]
    assert {1, 5, 130} <= {c["Nq"] for c in d4}
    assert any(c["Nq"] == 130 and c["causal"] and not K.packs(c) for c in d4), "the second 128-row query block, causal"
    assert any(K.packs(c) and 128 < c["Nq"] * G(c) <= 136 for c in d4), "packed rows just over one block"
    assert any(c["causal"] and any(n < nq for n, (_, nq) in zip(c["lens"], K.rows_of(c)[0]) if nq) for c in cs), "rows that see no key"
    assert {c["page"] for c in cs} >= {0, 64, 128, 256}
    assert {c["splits"] for c in cs} >= {0, 1, 2, 3, 4}
    assert any(c["splits"] == 4 and 65 in c["lens"] for c in cs), "trailing chunks empty"
    assert any(c["fp8"] and c["page"] for c in cs) and any(c["fp8"] and not c["page"] for c in cs)
    assert {c["pack"] for c in cs} == {None, True, False}
    pk = [c for c in cs if c["form"] == "packed"]
    assert pk and all(c["lq"] == [300, 1, 130, 0, 64] for c in pk)
    plain = [c for c in pk if c["append"] is None]
    assert all(0 in c["lens"] and c["cap"] in c["lens"] and any(n < q for n, q in zip(c["lens"], c["lq"])) for c in plain if c["max_q"] == 300)
    assert any(c["max_q"] < max(c["lq"]) for c in pk)
    assert sum(1 for c in cs if c["sched"]) >= 3 and any(c["sched"] and c["fp8"] for c in cs)
    assert {(c["append"], c["fp8"]) for c in cs if c["append"]} == {("4d", False), ("4d", True), ("varlen", False), ("varlen", True)}


def test_fp8_descales_differ_pairwise():
    for c in K.CASES:
        if not c["fp8"]:
            continue
        t, _ = _reference(c["id"], c["dtype"])
        for d in (t["kd"], t["vd"]):
            v = sorted(d.flatten().tolist())
            assert all(b / a >= 1.5 - 1e-6 for a, b in zip(v, v[1:])), c["id"]
        for cache in (t["k_cache"], t["v_cache"]):      # NaN codes behind every length (and where an append will write)
            for b in range(t["B"]):
                n = int(t["lens_call"][b])
                tail = K.gather(cache, t["bt"], b, c["cap"])[n:]
                assert bool(torch.isnan(tail).all()), c["id"]


def test_lse_bound_is_small():
    """The derived bound against the bar the family's other tests use (1e-4 * max(1, |lse|)): well below it on every case."""
    worst = 0.0
    for c in K.CASES:
        t, ref = _reference(c["id"], c["dtype"])
        for b, (_, lse, _, T, n) in ref.items():
            fin = torch.isfinite(lse)
            if fin.any():
                worst = max(worst, (K.lse_bound(T[fin], n, lse[fin], c["D"], K.lse_splits(c)) / (1e-4 * lse[fin].abs().clamp_min(1.0))).max().item())
    print(f"largest LSE bound: {worst:.3f} of 1e-4 * max(1, |lse|)")
    assert worst < 1.0 and math.isfinite(worst)
