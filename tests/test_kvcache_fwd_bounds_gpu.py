"""The KV-cache forward family held to per-element rounding bounds (tests/kvcache_ref.py): every case runs the public call — flash_attn_with_kvcache in its
4-D form or with cu_seqlens_q / max_seqlen_q, through scheduler_metadata, k_descale / v_descale, pack_gqa and num_splits as the case names them, with k= / v=
or kvcache_append_varlen(q=, rotary tables) in front where it says so — and asserts, element by element and sequence by sequence against fp64 (never against
another run of the kernels):
    out   |out16 - ref| <= eps16 * A + 1e-6 + half an ulp16 of the result * (1 + 1e-3),   A = v_descale * sum_j P_ij |dec v_jd|
    lse   |lse - ref| <= kvcache_ref.lse_bound (a closed form in 2^-24 derived from the kernels' statements)
    a row that sees no key: lse = +inf exactly and out = 0 exactly;  no NaN anywhere.
tests/test_kvcache_bounds_cpu.py proves on the CPU that the correct algorithm fits both bounds on every case and that the mutants a case names miss one of
them by 10x.  max(|d| / bound) is printed per case before it is asserted (profiles/kvcache_fwd_bounds.txt).  An append is also compared with the bytes it
is defined to store.  Every table entry, length and cu_seqlens_q here is in range; the one nq_b above max_seqlen_q is the clamping the packed form defines.
"""
import functools

import pytest
import torch

import kvcache_ref as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """The case's tensors and the fp64 reference of every sequence with rows: computed once (the scheduled form of a case shares its case's), never modified."""
    c = K.case_of(case_id)
    if c["sched"] and case_id in K.BY_ID:
        t, ref = reference(case_id[:-len("-sched")])
        return dict(t, case=c), ref
    t = K.build(c)
    return t, K.reference(t)


def same_values(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def call(t, dev, place=None):
    """The public call(s) of a case; returns per sequence with rows (out (nq, H, D), lse (H, nq)) on the CPU.  place: (k_cache, v_cache, block_table) on the device
    to use instead of fresh copies of the case's (tests/test_far_pool_gpu.py; what an append leaves in them is then its caller's to compare)."""
    import tiny_flash_attention_amd as tfa

    c = t["case"]
    d = lambda x: None if x is None else x.to(dev)     # noqa: E731  (a fresh device copy: an append writes it)
    kc, vc, bt = (d(t["k_cache"]), d(t["v_cache"]), d(t["bt"])) if place is None else place
    q = d(t["q_call"])
    kd, vd = (d(t["kd"]), d(t["vd"])) if c["fp8"] else (None, None)
    kw = dict(block_table=bt, softmax_scale=t["sc"], causal=c["causal"], num_splits=c["splits"], return_softmax_lse=True, pack_gqa=c["pack"], k_descale=kd,
              v_descale=vd)
    with torch.no_grad():
        if c["form"] == "4d":
            B, Nq = t["B"], c["Nq"]
            out, lse = tfa.flash_attn_with_kvcache(q.view(B, Nq, c["H"], c["D"]), kc, vc, k=d(t["k_new"]), v=d(t["v_new"]), cache_seqlens=d(t["lens_call"]), **kw)
            torch.cuda.synchronize()
            assert tuple(out.shape) == (B, Nq, c["H"], c["D"]) and tuple(lse.shape) == (B, c["H"], Nq) and lse.dtype == torch.float32
            res = {b: (out[b].cpu(), lse[b].cpu()) for b in range(B) if t["rows"][b][1] > 0}
        else:
            cu = d(t["cu"])
            if c["append"] == "varlen":
                tfa.kvcache_append_varlen(d(t["k_new"]), d(t["v_new"]), kc, vc, cu, d(t["before"]), bt, rotary_cos=d(t["cos"]), rotary_sin=d(t["sin"]), q=q,
                                          k_descale=kd, v_descale=vd)
                torch.cuda.synchronize()
                assert same_values(q, t["q"]), "kvcache_append_varlen(q=): q is not the rows rotated at before_b + t"
            md = None
            if c["sched"]:
                md = tfa.get_scheduler_metadata(cu, c["max_q"], t["total_q"], c["H"], c["Hk"], causal=c["causal"], pack_gqa=c["pack"])
            out, lse = tfa.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=d(t["lens_call"]), cu_seqlens_q=cu, max_seqlen_q=c["max_q"], scheduler_metadata=md, **kw)
            torch.cuda.synchronize()
            assert tuple(out.shape) == tuple(q.shape) and tuple(lse.shape) == (c["H"], t["total_q"]) and lse.dtype == torch.float32
            out, lse = out.cpu(), lse.cpu()
            res = {b: (out[q0:q0 + nq], lse[:, q0:q0 + nq]) for b, (q0, nq) in enumerate(t["rows"]) if nq > 0}
    if c["append"] is not None and place is None:
        assert same_values(kc, t["k_final"]) and same_values(vc, t["v_final"]), "the caches behind the append are not what the append is defined to store"
    return res


def run_case(case_id, dev):
    t, ref = reference(case_id)
    check(case_id, t, ref, call(t, dev))


def check(case_id, t, ref, got):
    c = t["case"]
    assert set(got) == set(ref)
    wo = wl = 0.0
    empty = 0
    for b, (out, lse, A, T, n) in ref.items():
        o, l = got[b]
        what = f"{case_id}[seq {b}: {t['rows'][b][1]} rows x {n} keys]"
        assert not bool(torch.isnan(o).any()) and not bool(torch.isnan(l).any()), f"{what}: NaN"
        unseen = torch.isposinf(lse)                                       # (H, nq)
        assert torch.equal(torch.isposinf(l), unseen), f"{what}: lse = +inf on other rows than the definition's"
        assert bool((o.transpose(0, 1)[unseen] == 0).all()), f"{what}: out != 0 on a row that sees no key"
        empty += int(unseen.sum())
        ro, rl = K.out_ratio(o.double(), out, A, t["dtype"]), K.lse_ratio(l, lse, T, n, c["D"], K.lse_splits(c))
        print(f"{what}: max(|d| / bound) out {ro:.3f}  lse {rl:.4f}")
        wo, wl = max(wo, ro), max(wl, rl)
    print(f"{case_id} {'bf16' if t['dtype'] == torch.bfloat16 else 'fp16'}: max(|d| / bound) out {wo:.3f}  lse {wl:.4f}  (rows without a key: {empty})")
    assert wo <= 1.0, f"{case_id}: out is at {wo:.3f} of its per-element bound"
    assert wl <= 1.0, f"{case_id}: lse is at {wl:.3f} of its per-element bound"


@pytest.mark.parametrize("case_id", [c["id"] for c in K.CASES])
def test_case_vs_fp64_bounds(dev, case_id):
    run_case(case_id, dev)


@pytest.mark.parametrize("seed", range(48))
def test_seeded_sweep(dev, seed):
    case = K.sweep_case(seed)
    print({k: v for k, v in case.items() if k not in ("mutants", "na")})
    run_case(case["id"], dev)
