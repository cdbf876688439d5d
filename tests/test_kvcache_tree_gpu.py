"""flash_attn_with_kvcache(tree_mask=) held to the per-element bounds of tests/kvcache_ref.py on the definition of tests/kvcache_tree_ref.py: every case runs the
public call — 4-D or with cu_seqlens_q / max_seqlen_q, through scheduler_metadata, k_descale / v_descale, pack_gqa, num_splits, k= / v= and
kvcache_append_varlen as the case names them — and asserts, element by element against fp64 (never against another run of the kernels):
    out   |out16 - ref| <= eps16 * A + 1e-6 + half an ulp16 of the result,   A summed over the keys the mask leaves
    lse   |lse - ref| <= kvcache_ref.lse_bound
    a row that sees no key: lse = +inf exactly and out = 0 exactly;  no NaN anywhere.
tests/test_kvcache_tree_bounds_cpu.py proves on the CPU that the correct algorithm fits both bounds and that every tree mutant misses one by 10x.  Then: bit
identity (all-ones words vs the plain causal call, scheduled vs unscheduled, a strided (B, Nq) mask and the bool form vs contiguous words), a cleared bit below 64
on rows from the 64th on, and a captured append + attention step replayed after the mask, the lengths, cu_seqlens_q and the new rows were overwritten in place.
max(|d| / bound) is printed per case before it is asserted (profiles/kvcache_tree_bounds.txt).
"""
import functools

import pytest
import torch

import kvcache_ref as K
import kvcache_tree_ref as T

pytestmark = pytest.mark.gpu
GPU_SWEEP = 16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """The case's tensors and the fp64 reference of every sequence with rows: computed once (the scheduled form of a case shares its case's), never modified."""
    c = T.case_of(case_id)
    if c["sched"] and case_id in T.BY_ID:
        t, ref = reference(case_id[:-len("-sched")])
        return dict(t, case=c), ref
    t = T.build(c)
    return t, T.reference(t)


def same_values(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def call(t, dev, mask="words", sched=None, place=None):
    """The public call of a case.  mask: "words" (the case's int64 words, contiguous), "strided" (the same words inside a wider tensor), "bool" (4-D: the bool
    form), "ones" (all-ones words) or None (the plain causal call).  place: (k_cache, v_cache, block_table) on the device to use instead of fresh copies of the case's
    (tests/test_far_pool_gpu.py; what an append leaves in them is then its caller's to compare).  Returns per sequence with rows (out (nq, H, D), lse (H, nq)) on the CPU."""
    import tiny_flash_attention_amd as tfa

    c = t["case"]
    d = lambda x: None if x is None else x.to(dev)     # noqa: E731  (a fresh device copy: an append writes it)
    kc, vc, bt = (d(t["k_cache"]), d(t["v_cache"]), d(t["bt"])) if place is None else place
    q = d(t["q_call"])
    kd, vd = (d(t["kd"]), d(t["vd"])) if c["fp8"] else (None, None)
    B, packed = t["B"], c["form"] == "packed"
    words = t["words"] if packed else t["words"].view(B, c["Nq"])
    if mask is None:
        tm = None
    elif mask == "ones":
        tm = torch.full_like(words, -1).to(dev)
    elif mask == "strided":
        wide = torch.full(tuple(words.shape) + (3,), 0x5555, dtype=torch.int64)
        wide = torch.cat([wide, wide], dim=-2)             # twice the rows, three words per row: the case's words at [..., :rows, 1]
        wide[..., :words.shape[-1], 1] = words
        tm = wide.to(dev)[..., :words.shape[-1], 1]
        assert not tm.is_contiguous()
    elif mask == "bool":
        tm = T.bool_of(words, c["Nq"]).to(dev)
    else:
        tm = words.to(dev)
    kw = dict(block_table=bt, softmax_scale=t["sc"], causal=True, num_splits=c["splits"], return_softmax_lse=True, pack_gqa=c["pack"], k_descale=kd, v_descale=vd)
    if tm is not None:
        kw["tree_mask"] = tm
    with torch.no_grad():
        if not packed:
            Nq = c["Nq"]
            out, lse = tfa.flash_attn_with_kvcache(q.view(B, Nq, c["H"], c["D"]), kc, vc, k=d(t["k_new"]), v=d(t["v_new"]), cache_seqlens=d(t["lens_call"]), **kw)
            torch.cuda.synchronize()
            assert tuple(out.shape) == (B, Nq, c["H"], c["D"]) and tuple(lse.shape) == (B, c["H"], Nq) and lse.dtype == torch.float32
            res = {b: (out[b].cpu(), lse[b].cpu()) for b in range(B) if t["rows"][b][1] > 0}
        else:
            cu = d(t["cu"])
            if c["append"] == "varlen":
                tfa.kvcache_append_varlen(d(t["k_new"]), d(t["v_new"]), kc, vc, cu, d(t["before"]), bt, rotary_cos=d(t["cos"]), rotary_sin=d(t["sin"]), q=q,
                                          k_descale=kd, v_descale=vd)
            md = None
            if c["sched"] if sched is None else sched:
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
    for b, (out, lse, A, Tm, n) in ref.items():
        o, l = got[b]
        what = f"{case_id}[seq {b}: {t['rows'][b][1]} rows x {t['lens'][b]} keys]"
        assert not bool(torch.isnan(o).any()) and not bool(torch.isnan(l).any()), f"{what}: NaN"
        unseen = torch.isposinf(lse)                                       # (H, nq)
        assert torch.equal(torch.isposinf(l), unseen), f"{what}: lse = +inf on other rows than the definition's"
        assert bool((o.transpose(0, 1)[unseen] == 0).all()), f"{what}: out != 0 on a row that sees no key"
        empty += int(unseen.sum())
        ro, rl = K.out_ratio(o.double(), out, A, t["dtype"]), K.lse_ratio(l, lse, Tm, n, c["D"], K.lse_splits(c))
        wo, wl = max(wo, ro), max(wl, rl)
    print(f"{case_id} {'bf16' if t['dtype'] == torch.bfloat16 else 'fp16'} {c['mask']}: max(|d| / bound) out {wo:.3f}  lse {wl:.4f}  (rows without a key: {empty})")
    assert wo <= 1.0, f"{case_id}: out is at {wo:.3f} of its per-element bound"
    assert wl <= 1.0, f"{case_id}: lse is at {wl:.3f} of its per-element bound"


def identical(x, y):
    assert set(x) == set(y)
    return all(same_values(x[b][0], y[b][0]) and same_values(x[b][1], y[b][1]) for b in x)


# ---- 1. every case and the draws against the two bounds -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", [c["id"] for c in T.CASES])
def test_case_vs_fp64_bounds(dev, case_id):
    t, ref = reference(case_id)
    check(case_id, t, ref, call(t, dev))


@pytest.mark.parametrize("seed", range(GPU_SWEEP))
def test_seeded_sweep(dev, seed):
    case = T.sweep_case(seed)
    print({k: v for k, v in case.items() if k not in ("mutants", "na", "tmutants", "tna")})
    t, ref = reference(case["id"])
    check(case["id"], t, ref, call(t, dev))


# ---- 2. bit identity ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", [c["id"] for c in T.CASES if c["form"] == "packed" or c["Nq"] > 1])
def test_all_ones_words_are_the_plain_causal_call_bit_for_bit(dev, case_id):
    """The same form, pack_gqa, layout and split count, more than one row per sequence: the tree kernel with nothing masked runs the plain kernel's arithmetic."""
    t, _ = reference(case_id)
    assert identical(call(t, dev, mask="ones"), call(t, dev, mask=None)), f"{case_id}: all-ones words change the arithmetic"


@pytest.mark.parametrize("case_id", [c["id"] for c in T.CASES if c["sched"]])
def test_scheduled_equals_unscheduled_bit_for_bit(dev, case_id):
    t, _ = reference(case_id)
    assert identical(call(t, dev), call(t, dev, sched=False)), f"{case_id}: a block's arithmetic depends on the work item that runs it"


@pytest.mark.parametrize("case_id", ["t4d-bf16-d40-g1-nq40-tree", "t4d-fp16-d128-g4-nq64-s2-pack", "t4d-fp8-bf16-d48-g2-nq5", "t4d-bf16-d64-g8-nq1-page256",
                                     "tvq-bf16-d64-g4-tree"])
def test_a_strided_mask_and_the_bool_form_are_the_same_call(dev, case_id):
    t, ref = reference(case_id)
    base = call(t, dev)
    got = call(t, dev, mask="strided")
    check(case_id + " (strided words)", t, ref, got)
    assert identical(got, base)
    if t["case"]["form"] == "4d":
        assert identical(call(t, dev, mask="bool"), base), f"{case_id}: the bool form is not the int64 form"


@pytest.mark.parametrize("case_id", ["tvq-fp16-d128-g2-page128-s3-unpacked-longclear", "tvq-bf16-d40-g1-page64-s2-maxq128"])
def test_a_cleared_bit_below_64_bites_on_rows_from_the_64th_on(dev, case_id):
    """The long rows' words hide one of the sequence's first 64 new keys: their out differs from the all-ones call's, and (test_case_vs_fp64_bounds) is the definition's."""
    t, _ = reference(case_id)
    got, ones = call(t, dev), call(t, dev, mask="ones")
    long = [b for b, (_, nq) in enumerate(t["rows"]) if nq > 64]
    assert long
    for b in long:
        nq = t["rows"][b][1]
        assert not same_values(got[b][0][64:nq], ones[b][0][64:nq]), f"{case_id}: the mask does not reach rows 64.. of sequence {b}"


# ---- 3. a captured step ------------------------------------------------------------------------------------------------------------------------------------------
def test_captured_append_and_attention_see_what_was_overwritten_in_place(dev):
    """kvcache_append_varlen + the packed tree call, captured once; each replay follows an in-place overwrite of the words, the lengths, cu_seqlens_q and the new
    rows, and is compared bit for bit with an eager call on a copy of the caches as they were in front of the replay."""
    import tiny_flash_attention_amd as tfa

    g = torch.Generator().manual_seed(91)
    dtype, B, H, Hk, D, cap, page, total = torch.bfloat16, 2, 8, 2, 64, 256, 64, 12
    mb = cap // page
    bt = torch.randperm(B * mb, generator=g).view(B, mb).to(torch.int32).to(dev)
    kc, vc = (torch.randn(B * mb, page, Hk, D, generator=g).mul(0.5).to(dtype).to(dev) for _ in range(2))
    steps = []
    for nqs, before in (([5, 7], [60, 100]), ([8, 4], [120, 61]), ([1, 11], [200, 59])):
        c = T._case("cap", "tree", form="packed", lq=nqs, lens=[b + n for b, n in zip(before, nqs)], cap=cap, H=H, Hk=Hk, D=D, seed=90 + nqs[0])
        steps.append(dict(q=torch.randn(total, H, D, generator=g).to(dtype), k=torch.randn(total, Hk, D, generator=g).mul(0.5).to(dtype),
                          v=torch.randn(total, Hk, D, generator=g).mul(0.5).to(dtype), cu=torch.tensor([0, nqs[0], total], dtype=torch.int32),
                          before=torch.tensor(before, dtype=torch.int32), lens=torch.tensor(c["lens"], dtype=torch.int32),
                          words=torch.tensor([w for ws in T.words_of(c) for w in ws], dtype=torch.int64)))
    s = {k: v.to(dev).clone() for k, v in steps[0].items()}

    def step(x, kc_, vc_):
        tfa.kvcache_append_varlen(x["k"], x["v"], kc_, vc_, x["cu"], x["before"], bt)
        return tfa.flash_attn_with_kvcache(x["q"], kc_, vc_, cache_seqlens=x["lens"], block_table=bt, causal=True, num_splits=2, return_softmax_lse=True,
                                           cu_seqlens_q=x["cu"], max_seqlen_q=total, tree_mask=x["words"])

    with torch.no_grad():
        step(s, kc.clone(), vc.clone())                    # one warm-up call outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out_s, lse_s = step(s, kc, vc)
        outs = []
        for x in steps[1:] + steps[:1]:
            for k, v in x.items():
                s[k].copy_(v.to(dev))
            kc_e, vc_e = kc.clone(), vc.clone()
            graph.replay()
            torch.cuda.synchronize()
            out_e, lse_e = step({k: v.to(dev) for k, v in x.items()}, kc_e, vc_e)
            torch.cuda.synchronize()
            assert same_values(out_s, out_e) and same_values(lse_s, lse_e), "a replay does not see what was overwritten in place"
            assert same_values(kc, kc_e) and same_values(vc, vc_e)
            outs.append(out_s.cpu().clone())
        assert not same_values(outs[0], outs[1]) and not same_values(outs[1], outs[2])
    torch.cuda.synchronize()
