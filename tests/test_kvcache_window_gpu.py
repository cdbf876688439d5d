"""flash_attn_with_kvcache(sliding_window=w) held to the per-element bounds of tests/kvcache_window_ref.py: every case runs the public call — 4-D or with
cu_seqlens_q / max_seqlen_q, through scheduler_metadata, k_descale / v_descale, pack_gqa, num_splits and k= / v= as the case names them — and asserts, element
by element against fp64 (never against another run of the kernels):
    out   |out16 - ref| <= eps16 * A + 1e-6 + half an ulp16 of the result,   A summed over the window's keys
    lse   |lse - ref| <= kvcache_ref.lse_bound with the tiles of [lo64_b, len_b)
    a row that sees no key: lse = +inf exactly and out = 0 exactly;  no NaN anywhere.
tests/test_kvcache_window_bounds_cpu.py proves on the CPU that the correct algorithm fits both bounds and that every window mutant misses one by 10x.  Then:
bit identity (scheduled vs unscheduled; a window that reaches every key vs the plain causal call), the touch promise (pages wholly in front of lo64_b hold NaN,
their table entries are out of range — where the header promises they are not read), and a captured decode step whose window moves between the replays.
max(|d| / bound) is printed per case before it is asserted (profiles/kvcache_window_bounds.txt).
"""
import functools
import math

import pytest
import torch

import kvcache_ref as K
import kvcache_window_ref as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """The case's tensors and the fp64 reference of every sequence with rows: computed once (the scheduled form of a case shares its case's), never modified."""
    c = W.case_of(case_id)
    if c["sched"] and case_id in W.BY_ID:
        t, ref = reference(case_id[:-len("-sched")])
        return dict(t, case=c), ref
    t = W.build(c)
    return t, W.reference(t)


def same_values(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def call(t, dev, window="case", kc=None, vc=None, bt=None, splits=None, place=None):
    """The public call of a case (window: the case's w, None = the plain causal call, or another w; kc / vc / bt: device tensors to use instead of fresh copies of
    the case's; place: all three at once, as tests/test_far_pool_gpu.py hands them over — what an append leaves in them is then its caller's to compare); returns per sequence with rows (out (nq, H, D), lse (H, nq)) on the CPU."""
    import tiny_flash_attention_amd as tfa

    c = t["case"]
    d = lambda x: None if x is None else x.to(dev)     # noqa: E731  (a fresh device copy: an append writes it)
    if place is not None:
        kc, vc, bt = place
    kc = d(t["k_cache"]) if kc is None else kc
    vc = d(t["v_cache"]) if vc is None else vc
    bt = d(t["bt"]) if bt is None else bt
    q = d(t["q_call"])
    kd, vd = (d(t["kd"]), d(t["vd"])) if c["fp8"] else (None, None)
    kw = dict(block_table=bt, softmax_scale=t["sc"], causal=True, num_splits=c["splits"] if splits is None else splits, return_softmax_lse=True, pack_gqa=c["pack"],
              k_descale=kd, v_descale=vd, sliding_window=c["w"] if window == "case" else window)
    with torch.no_grad():
        if c["form"] == "4d":
            B, Nq = t["B"], c["Nq"]
            out, lse = tfa.flash_attn_with_kvcache(q.view(B, Nq, c["H"], c["D"]), kc, vc, k=d(t["k_new"]), v=d(t["v_new"]), cache_seqlens=d(t["lens_call"]), **kw)
            torch.cuda.synchronize()
            assert tuple(out.shape) == (B, Nq, c["H"], c["D"]) and tuple(lse.shape) == (B, c["H"], Nq) and lse.dtype == torch.float32
            res = {b: (out[b].cpu(), lse[b].cpu()) for b in range(B) if t["rows"][b][1] > 0}
        else:
            cu = d(t["cu"])
            md = None
            if c["sched"]:
                md = tfa.get_scheduler_metadata(cu, c["max_q"], t["total_q"], c["H"], c["Hk"], causal=True, pack_gqa=c["pack"])
            out, lse = tfa.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=d(t["lens_call"]), cu_seqlens_q=cu, max_seqlen_q=c["max_q"], scheduler_metadata=md, **kw)
            torch.cuda.synchronize()
            assert tuple(out.shape) == tuple(q.shape) and tuple(lse.shape) == (c["H"], t["total_q"]) and lse.dtype == torch.float32
            out, lse = out.cpu(), lse.cpu()
            res = {b: (out[q0:q0 + nq], lse[:, q0:q0 + nq]) for b, (q0, nq) in enumerate(t["rows"]) if nq > 0}
    if c["append"] is not None and place is None:
        assert same_values(kc, t["k_final"]) and same_values(vc, t["v_final"]), "the caches behind the append are not what the append is defined to store"
    return res


def check(case_id, t, ref, got):
    c = t["case"]
    assert set(got) == set(ref)
    wo = wl = 0.0
    empty = 0
    for b, (out, lse, A, T, n) in ref.items():
        o, l = got[b]
        what = f"{case_id}[seq {b}: {t['rows'][b][1]} rows x {t['lens'][b]} keys, w {c['w']}]"
        assert not bool(torch.isnan(o).any()) and not bool(torch.isnan(l).any()), f"{what}: NaN"
        unseen = torch.isposinf(lse)                                       # (H, nq)
        assert torch.equal(torch.isposinf(l), unseen), f"{what}: lse = +inf on other rows than the definition's"
        assert bool((o.transpose(0, 1)[unseen] == 0).all()), f"{what}: out != 0 on a row that sees no key"
        empty += int(unseen.sum())
        ro, rl = K.out_ratio(o.double(), out, A, t["dtype"]), K.lse_ratio(l, lse, T, n, c["D"], K.lse_splits(c))
        wo, wl = max(wo, ro), max(wl, rl)
    print(f"{case_id} {'bf16' if t['dtype'] == torch.bfloat16 else 'fp16'} w={c['w']}: max(|d| / bound) out {wo:.3f}  lse {wl:.4f}  (rows without a key: {empty})")
    assert wo <= 1.0, f"{case_id}: out is at {wo:.3f} of its per-element bound"
    assert wl <= 1.0, f"{case_id}: lse is at {wl:.3f} of its per-element bound"


def run_case(case_id, dev):
    t, ref = reference(case_id)
    got = call(t, dev)
    check(case_id, t, ref, got)
    return got


# ---- 1. every case and the draws against the two bounds -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", [c["id"] for c in W.CASES])
def test_case_vs_fp64_bounds(dev, case_id):
    run_case(case_id, dev)


@pytest.mark.parametrize("seed", range(W.SWEEP))
def test_seeded_sweep(dev, seed):
    case = W.sweep_case(seed)
    print({k: v for k, v in case.items() if k not in ("mutants", "na", "wmutants", "wna")})
    run_case(case["id"], dev)


# ---- 2. bit identity ------------------------------------------------------------------------------------------------------------------------------------------
def identical(x, y):
    assert set(x) == set(y)
    return all(same_values(x[b][0], y[b][0]) and same_values(x[b][1], y[b][1]) for b in x)


@pytest.mark.parametrize("case_id", [c["id"] for c in W.CASES if c["sched"]])
def test_scheduled_equals_unscheduled_bit_for_bit(dev, case_id):
    t, _ = reference(case_id)
    base, _ = reference(case_id[:-len("-sched")])
    assert identical(call(t, dev), call(base, dev)), f"{case_id}: a block's arithmetic depends on the work item that runs it"


@pytest.mark.parametrize("case_id", ["w4d-fp16-d64-g2-nq5-w2-page64-s2", "w4d-bf16-d104-g4-nq1-w64-page128-s3", "wvq-fp8-fp16-d112-g2-w65-page256-pack",
                                     "wvq-bf16-d64-g4-w128-sched"])
def test_a_window_beyond_the_capacity_is_the_plain_causal_call(dev, case_id):
    t, _ = reference(case_id)
    cap = t["case"]["cap"]
    plain = call(t, dev, window=None)
    assert identical(call(t, dev, window=cap + 1), plain) and identical(call(t, dev, window=cap + 12345), plain)


COVER = [
    W._case("cover-4d-bf16-nq5", 512, dtype=K.BF16, D=64, H=4, Hk=2, Nq=5, lens=[300, 65, 129, 1], cap=1024, page=64, seed=60),
    W._case("cover-4d-fp16-nq1-g4", 512, dtype=K.FP16, D=128, H=8, Hk=2, Nq=1, lens=[300, 64, 127], cap=1024, seed=61),
    W._case("cover-4d-fp8-nq33-pack", 512, dtype=K.BF16, D=64, H=8, Hk=2, Nq=33, lens=[300, 128, 65], cap=1024, page=128, pack=True, fp8=True, seed=62),
    W._packed("cover-vq-fp16", 512, dtype=K.FP16, D=64, H=4, Hk=2, lens=[300, 128, 129, 65, 64], cap=1024, page=256, seed=63),
]


@pytest.mark.parametrize("case", COVER, ids=[c["id"] for c in COVER])
def test_a_window_that_covers_every_length_runs_the_plain_arithmetic(dev, case):
    """w >= every len_b but below the capacity: the windowed kernels run (w - 1 < capacity), lo64_b = 0 for every sequence, the ranges are the plain call's — so at
    num_splits = 1 the arithmetic is, bit for bit."""
    assert case["w"] - 1 < case["cap"] and all(n <= case["w"] for n in case["lens"]) and case["splits"] == 1
    t = W.build(case)
    assert identical(call(t, dev), call(t, dev, window=None))


# ---- 3. the touch promise -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("Nq", [1, 5])
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_pages_in_front_of_the_window_are_not_touched(dev, fp8, Nq, splits):
    """Every page wholly in front of lo64_b holds NaN (the NaN code in an fp8 cache) and its block-table entry is -1 or num_pages + 7: the header promises that
    neither is read.  out / lse must be finite where the reference is, and inside the bounds.  (Nothing here provokes a fault: a kernel that did read such an
    entry would clamp it into the pool, as every form does, and gather a wrong — NaN or foreign — page.)"""
    page = 64 if Nq == 1 else 128
    c = W._case(f"touch-{'fp8' if fp8 else '16'}-nq{Nq}-s{splits}", 100, dtype=K.BF16 if Nq == 1 else K.FP16, D=64, H=8, Hk=2, Nq=Nq, lens=[700, 1024, 300, 129, 65],
                cap=1024, page=page, splits=splits, fp8=fp8, seed=70 + Nq + splits)
    t = W.build(c)
    ref = W.reference(t)                                   # of the clean tensors: the definition does not read what the window hides
    kc, vc, bt = t["k_cache"].clone(), t["v_cache"].clone(), t["bt"].clone()
    num_pages, freed = kc.shape[0], 0
    for b, n in enumerate(t["lens"]):
        lo64 = W.lo64_of(n, Nq, c["w"] - 1)
        for i in range(lo64 // page):                      # pages [i * page, (i + 1) * page) that end at or before lo64_b
            for pool in (kc, vc):
                if fp8:
                    pool.view(torch.uint8)[int(bt[b, i])] = 0x7F
                else:
                    pool[int(bt[b, i])] = float("nan")
            bt[b, i] = -1 if i % 2 == 0 else num_pages + 7
            freed += 1
    assert freed >= 10
    got = call(t, dev, kc=kc.to(dev), vc=vc.to(dev), bt=bt.to(dev))
    check(c["id"], t, ref, got)


# ---- 4. a captured decode step whose window moves -----------------------------------------------------------------------------------------------------------
def test_captured_decode_step_with_a_moving_window(dev):
    """append + attention with w = 65 over pages of 64, captured once; replays at lengths 128, 129 and 130 after cache_seqlens.add_(1): the window's first key is
    63, 64, 65 — its first tile and page move from 0 to 1 between the first two replays — and every replay is checked against fp64."""
    import tiny_flash_attention_amd as tfa

    g = torch.Generator().manual_seed(81)
    dtype, B, H, Hk, D, cap, page, w = torch.bfloat16, 2, 8, 2, 64, 256, 64, 65
    sc = 1.0 / math.sqrt(D)
    mb = cap // page
    bt = torch.randperm(B * mb, generator=g).view(B, mb).to(torch.int32)
    kfull, vfull = torch.randn(B, cap, Hk, D, generator=g).mul(0.5).to(dtype), torch.randn(B, cap, Hk, D, generator=g).mul(0.5).to(dtype)
    qs = torch.randn(4, B, 1, H, D, generator=g).to(dtype)
    before = 127
    kpool, vpool = (torch.randn(B * mb, page, Hk, D, generator=g).mul(3.0).to(dtype) for _ in range(2))      # garbage wherever nothing was appended yet
    for b in range(B):
        for j in range(before):
            kpool[int(bt[b, j // page]), j % page] = kfull[b, j]
            vpool[int(bt[b, j // page]), j % page] = vfull[b, j]
    kc, vc, btd = kpool.to(dev), vpool.to(dev), bt.to(dev)
    seq = torch.full((B,), before, dtype=torch.int32, device=dev)
    q_s, k_s, v_s = qs[0].to(dev).clone(), kfull[:, before:before + 1].to(dev).clone(), vfull[:, before:before + 1].to(dev).clone()
    step = lambda: tfa.flash_attn_with_kvcache(q_s, kc, vc, k=k_s, v=v_s, cache_seqlens=seq, block_table=btd, causal=True, num_splits=1,      # noqa: E731
                                               return_softmax_lse=True, sliding_window=w)
    with torch.no_grad():
        step()                                             # one warm-up call outside the capture (it appends the first replay's row)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out_s, lse_s = step()
        for r, n in enumerate((128, 129, 130)):
            q_s.copy_(qs[r + 1].to(dev))
            k_s.copy_(kfull[:, n - 1:n].to(dev))
            v_s.copy_(vfull[:, n - 1:n].to(dev))
            graph.replay()
            torch.cuda.synchronize()
            out, lse = out_s.cpu(), lse_s.cpu()
            lo = n - 1 - (w - 1)
            assert (lo & ~63) // page == (0, 1, 1)[r]
            for b in range(B):
                q = qs[r + 1][b, 0].double()                                                  # (H, D)
                k = kfull[b, lo:n].double().repeat_interleave(H // Hk, dim=1).transpose(0, 1)  # (H, w, D)
                v = vfull[b, lo:n].double().repeat_interleave(H // Hk, dim=1).transpose(0, 1)
                s = torch.einsum("hd,hkd->hk", q, k) * sc
                P = torch.softmax(s, dim=-1)
                ref_o, ref_A = torch.einsum("hk,hkd->hd", P, v), torch.einsum("hk,hkd->hd", P, v.abs())
                ref_l = torch.logsumexp(s, dim=-1)
                T = (torch.einsum("hd,hkd->hk", q.abs(), k.abs()) * sc).max(dim=-1).values
                ro = K.out_ratio(out[b, 0].double(), ref_o, ref_A, dtype)
                rl = K.lse_ratio(lse[b, :, 0], ref_l, T, n - (lo & ~63), D, 1)
                print(f"replay at length {n}, sequence {b}: max(|d| / bound) out {ro:.3f}  lse {rl:.4f}")
                assert ro <= 1.0 and rl <= 1.0, (n, b, ro, rl)
            seq.add_(1)                                    # the caller advances the lengths, in place on the device
    torch.cuda.synchronize()
