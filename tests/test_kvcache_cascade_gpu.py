"""flash_attn_with_kvcache_cascade held to the per-element bounds of tests/kvcache_cascade_ref.py: every case runs the public call over a pool whose every byte behind a
length is NaN and asserts, element by element against the fp64 definition (never against another run of the kernels):
    out   |out16 - ref| <= eps16 * A + 1e-6 + half an ulp16 of the result,   A over the union of the row's shared and own keys
    lse   |lse - ref| <= kvcache_ref.lse_bound for ns0 + ns1 parts
    a row that sees no key — a row in no sequence and no group among them —: lse = +inf exactly and out = 0 exactly;  no NaN anywhere.
tests/test_kvcache_cascade_bounds_cpu.py proves on the CPU that the correct algorithm fits both bounds and that every mutant misses one by 10x.  Then: the scheduled
levels bit for bit the unscheduled ones, the flat packed-q call over full tables within the same bounds where that call is the same definition, the C entry point over
a NaN-filled workspace with canaries around out, lse, the workspace and the pool, and a captured call replayed after all six device arrays and the pool were
overwritten in place.  max(|d| / bound) is printed per case before it is asserted (profiles/kvcache_cascade_bounds.txt).
"""
import ctypes as C
import functools
import math

import pytest
import torch

import form_ref as F
import kvcache_cascade_ref as CR
import kvcache_ref as K

pytestmark = pytest.mark.gpu
GPU_SWEEP = 6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """The case's tensors (NaN behind every length) and its fp64 reference: computed once, never modified; a scheduled case shares its case's."""
    c = CR.case_of(case_id)
    if c["sched"] and case_id in CR.BY_ID:
        t, ref = reference(case_id[:-len("-sched")])
        return dict(t, case=c), ref
    t = CR.build(c, nan=True)
    return t, CR.reference(t)


def same_values(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def call(t, dev, sched=None, x=None):
    """The public call of a case; x: the device tensors to use instead of fresh copies.  (out (total_q, H, D), lse (H, total_q)) on the device."""
    import tiny_flash_attention_amd as tfa

    c = t["case"]
    x = x or {k: t[k].to(dev) for k in ("q", "k", "v", "bt", "pbt", "cu", "lens", "pcu", "plens")}
    md = pmd = None
    if c["sched"] if sched is None else sched:
        md = tfa.get_scheduler_metadata(x["cu"], t["max_q"], t["total_q"], c["H"], c["Hk"], causal=c["causal"], pack_gqa=c["pack"])
        pmd = tfa.get_scheduler_metadata(x["pcu"], t["pmax_q"], t["total_q"], c["H"], c["Hk"], causal=False, pack_gqa=c["pack"])
    with torch.no_grad():
        out, lse = tfa.flash_attn_with_kvcache_cascade(
            x["q"], x["k"], x["v"], cu_seqlens_q=x["cu"], max_seqlen_q=t["max_q"], cache_seqlens=x["lens"], block_table=x["bt"], prefix_cu_seqlens_q=x["pcu"],
            prefix_max_seqlen_q=t["pmax_q"], prefix_seqlens=x["plens"], prefix_block_table=x["pbt"], softmax_scale=t["sc"], causal=c["causal"],
            num_splits=c["splits"][1], prefix_num_splits=c["splits"][0], return_softmax_lse=True, pack_gqa=c["pack"], scheduler_metadata=md,
            prefix_scheduler_metadata=pmd)
    assert tuple(out.shape) == (t["total_q"], c["H"], c["D"]) and tuple(lse.shape) == (c["H"], t["total_q"]) and lse.dtype == torch.float32
    return out, lse


def check(case_id, t, ref, out, lse):
    out, lse = out.cpu(), lse.cpu()
    assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(lse).any()), f"{case_id}: NaN"
    unseen = torch.isposinf(ref[1])                                       # (H, total_q)
    assert torch.equal(torch.isposinf(lse), unseen), f"{case_id}: lse = +inf on other rows than the definition's"
    assert bool((out.transpose(0, 1)[unseen] == 0).all()), f"{case_id}: out != 0 on a row that sees no key"
    wo, wl = CR.ratios(t, out, lse, ref)
    print(f"{case_id}: max(|d| / bound) out {wo:.3f}  lse {wl:.4f}  ({sum(CR.chunks_of(t))} parts, rows without a key: {int(unseen.sum())})")
    assert wo <= 1.0, f"{case_id}: out is at {wo:.3f} of its per-element bound"
    assert wl <= 1.0, f"{case_id}: lse is at {wl:.3f} of its per-element bound"


# ---- 1. every case and the draws against the two bounds ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", [c["id"] for c in CR.CASES])
def test_case_vs_fp64_bounds(dev, case_id):
    t, ref = reference(case_id)
    check(case_id, t, ref, *call(t, dev))


@pytest.mark.parametrize("seed", range(GPU_SWEEP))
def test_seeded_sweep(dev, seed):
    case = CR.sweep_case(seed)
    print({k: v for k, v in case.items() if k not in ("mutants", "na")})
    t, ref = reference(case["id"])
    check(case["id"], t, ref, *call(t, dev))


# ---- 2. the work lists change nothing ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", [c["id"] for c in CR.CASES if c["sched"]])
def test_scheduled_equals_unscheduled_bit_for_bit(dev, case_id):
    t, _ = reference(case_id)
    (o1, l1), (o2, l2) = call(t, dev, sched=True), call(t, dev, sched=False)
    assert same_values(o1, o2) and same_values(l1, l2), f"{case_id}: a block's arithmetic depends on the work item that runs it"


# ---- 3. the flat packed-q call ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", [c["id"] for c in CR.CASES[:4]])
def test_flat_packed_q_call_is_within_the_same_bounds(dev, case_id):
    """Where the flat call over full tables is the same definition (plen_g a page multiple, ulen_b >= nq_b), it lies within the bounds of the cascade's reference —
    and so within twice the out bound of the cascade call."""
    import tiny_flash_attention_amd as tfa

    t, ref = reference(case_id)
    c = t["case"]
    ft, same = CR.flat(t)
    out, lse = (x.cpu() for x in call(t, dev))
    with torch.no_grad():
        fo, fl = tfa.flash_attn_with_kvcache(t["q"].to(dev), t["k"].to(dev), t["v"].to(dev), cache_seqlens=torch.tensor(ft["lens"], dtype=torch.int32).to(dev),
                                             block_table=ft["bt"].to(dev), softmax_scale=t["sc"], causal=c["causal"], num_splits=1, return_softmax_lse=True,
                                             pack_gqa=c["pack"], cu_seqlens_q=t["cu"].to(dev), max_seqlen_q=t["max_q"])
    fo, fl = fo.cpu(), fl.cpu()
    checked = 0
    ro, rl, A, T, n = ref
    for b, (q0, nq) in enumerate(ft["rows"]):
        if not same[b] or nq == 0:
            continue
        s = slice(q0, q0 + nq)
        wo = K.out_ratio(fo[s].double(), ro[s], A[s], t["dtype"])
        b1 = F.eps16(t["dtype"]) * A[s] + 1e-6               # both calls lie within b1 + half an ulp16 of ref (form_ref.ratios): their difference within twice that
        bound = b1 + 0.5 * F.ulp16((ro[s].abs() + b1).float(), t["dtype"]).double() * (1 + 1e-3)
        d = ((fo[s].double() - out[s].double()).abs() / (2 * bound)).max().item()
        fin = torch.isfinite(rl[:, s])
        assert torch.equal(torch.isposinf(fl[:, s]), ~fin)
        wl = ((fl[:, s].double() - rl[:, s]).abs()[fin] / K.lse_bound(T[:, s], n[s].view(1, -1), rl[:, s], c["D"], 1)[fin]).max().item() if bool(fin.any()) else 0.0
        print(f"{case_id}[seq {b}]: the flat call at {wo:.3f} of the out bound, {wl:.4f} of the one-chunk LSE bound; flat vs cascade at {d:.3f} of twice the bound")
        assert wo <= 1.0 and wl <= 1.0 and d <= 1.0
        checked += 1
    assert checked >= 2


# ---- 4. the C entry point: a NaN workspace, canaries ------------------------------------------------------------------------------------------------------------
def _abi_call(t, dev, x, out, lse, ws, splits, pack):
    from tiny_flash_attention_amd import _lib

    c = t["case"]
    L = _lib.lib()
    H, Hk, D, total = c["H"], c["Hk"], c["D"], t["total_q"]
    p = _lib.TfaKvcacheParams()
    p.q, p.out, p.lse = x["q"].data_ptr(), out.data_ptr(), lse.data_ptr()
    p.k_cache, p.v_cache, p.cache_seqlens = x["k"].data_ptr(), x["v"].data_ptr(), x["lens"].data_ptr()
    p.B, p.H, p.Hk, p.Nq, p.D, p.capacity = t["B"], H, Hk, 0, D, t["cap1"]
    p.block_table, p.block_table_stride = x["bt"].data_ptr(), x["bt"].stride(0)
    p.page_size, p.num_pages = x["k"].shape[1], x["k"].shape[0]
    p.q_stride[0], p.q_stride[1], p.q_stride[2] = 0, x["q"].stride(1), x["q"].stride(0)
    p.o_stride[0], p.o_stride[1], p.o_stride[2] = 0, total * D, D
    for name, src in (("k_stride", x["k"]), ("v_stride", x["v"])):
        arr = getattr(p, name)
        arr[0], arr[1], arr[2] = src.stride(0), src.stride(2), src.stride(1)
    p.softmax_scale, p.is_causal, p.dtype = t["sc"], 1 if c["causal"] else 0, _lib.TFA_BF16 if t["dtype"] == torch.bfloat16 else _lib.TFA_F16
    vq = _lib.TfaKvcacheVarlenQ()
    vq.cu_seqlens_q, vq.max_seqlen_q, vq.total_q = x["cu"].data_ptr(), t["max_q"], total
    cs = _lib.TfaKvcacheCascade()
    cs.prefix_cu_seqlens_q, cs.prefix_seqlens, cs.prefix_block_table = x["pcu"].data_ptr(), x["plens"].data_ptr(), x["pbt"].data_ptr()
    cs.prefix_block_table_stride, cs.num_groups, cs.prefix_max_blocks, cs.prefix_max_seqlen_q = x["pbt"].stride(0), t["Gn"], x["pbt"].shape[1], t["pmax_q"]
    need = L.tfa_fwd_kvcache_cascade_workspace(C.byref(p), C.byref(vq), C.byref(cs), pack, splits[1], splits[0])
    assert need == sum(CR.chunks_of(t)) * H * total * (D + 1) and need <= ws.numel()
    st = L.tfa_fwd_kvcache_cascade(C.byref(p), C.byref(vq), C.byref(cs), pack, splits[1], splits[0], None, None, ws.data_ptr(),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0, _lib.strerror(st)
    torch.cuda.synchronize()
    return need


@pytest.mark.parametrize("case_id", ["cs-bf16-d64-h8k2-packTrue-p130_1_64-s32", "cs-fp16-d128-h4k4-packNone-p64_0_130-s12", "cs-bf16-d64-h8k2-packNone-p130_64_1-s11"])
def test_c_call_over_a_nan_workspace_writes_nothing_else(dev, case_id):
    """tfa_fwd_kvcache_cascade with every workspace word NaN on entry: the result is the public call's bit for bit (which the bounds hold), every word around out,
    lse and the workspace keeps its canary, and no byte of the pool changes."""
    from tiny_flash_attention_amd import _lib

    t, ref = reference(case_id)
    c = t["case"]
    H, D, total = c["H"], c["D"], t["total_q"]
    x = {k: t[k].to(dev) for k in ("q", "k", "v", "bt", "pbt", "cu", "lens", "pcu", "plens")}
    pool0 = (x["k"].clone(), x["v"].clone())
    PAD, CAN = 4096, -12345.0
    need = sum(CR.chunks_of(t)) * H * total * (D + 1)
    obuf = torch.full((PAD + H * total * D + PAD,), CAN, dtype=t["dtype"], device=dev)
    lbuf = torch.full((PAD + H * total + PAD,), CAN, dtype=torch.float32, device=dev)
    wbuf = torch.full((PAD + need + PAD,), CAN, dtype=torch.float32, device=dev)
    out, lse, ws = obuf[PAD:PAD + H * total * D], lbuf[PAD:PAD + H * total], wbuf[PAD:PAD + need]
    ws.fill_(math.nan)
    pack = _lib.TFA_PACK_GQA_OFF if c["pack"] is False else _lib.TFA_PACK_GQA_ON
    assert _abi_call(t, dev, x, out, lse, ws, c["splits"], pack) == need
    for buf, n in ((obuf, H * total * D), (lbuf, H * total), (wbuf, need)):
        assert bool((buf[:PAD] == CAN).all()) and bool((buf[PAD + n:] == CAN).all()), f"{case_id}: a word outside its tensor was written"
    assert same_values(x["k"].view(torch.int16), pool0[0].view(torch.int16)) and same_values(x["v"].view(torch.int16), pool0[1].view(torch.int16))
    o, l = out.view(H, total, D).transpose(0, 1), lse.view(H, total)
    check(case_id + " (C call, NaN workspace)", t, ref, o, l)
    po, pl = call(t, dev, sched=False)
    assert same_values(o, po) and same_values(l, pl), f"{case_id}: the result depends on what the workspace held"


# ---- 5. a captured call -----------------------------------------------------------------------------------------------------------------------------------------
def test_captured_call_sees_all_six_arrays_and_the_pool_overwritten_in_place(dev):
    order = ([0, 1, 2, 3, 4, 5, 6], [6, 3, 1, 0, 5, 2, 4], [2, 5, 0, 6, 3, 4, 1])
    steps = []
    for i, (perm, sizes, plens) in enumerate(zip(order, ((3, 1, 2), (2, 3, 1), (1, 2, 3)), ((130, 64, 1), (0, 130, 64), (64, 1, 130)))):
        c = CR._case(f"cap{i}", [CR.SEQS_B[j] for j in perm], list(zip(sizes, plens)), splits=(3, 2), seed=70 + i)
        steps.append(CR.build(c, nan=True))
    keys = ("q", "k", "v", "bt", "pbt", "cu", "lens", "pcu", "plens")
    assert all(tuple(s[k].shape) == tuple(steps[0][k].shape) for s in steps for k in keys)
    max_q, pmax_q = max(s["max_q"] for s in steps), max(s["pmax_q"] for s in steps)
    steps = [dict(s, max_q=max_q, pmax_q=pmax_q) for s in steps]
    x = {k: steps[0][k].to(dev).clone() for k in keys}
    with torch.no_grad():
        call(steps[0], dev, x=x)                           # one warm-up call outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out_s, lse_s = call(steps[0], dev, x=x)
        outs = []
        for s in steps[1:] + steps[:1]:
            for k in keys:
                x[k].copy_(s[k].to(dev))
            graph.replay()
            torch.cuda.synchronize()
            out_e, lse_e = call(s, dev)
            torch.cuda.synchronize()
            assert same_values(out_s, out_e) and same_values(lse_s, lse_e), "a replay does not see what was overwritten in place"
            check(s["case"]["id"] + " (replayed)", s, CR.reference(s), out_s, lse_s)
            outs.append(out_s.cpu().clone())
        assert not same_values(outs[0], outs[1]) and not same_values(outs[1], outs[2])
    torch.cuda.synchronize()
