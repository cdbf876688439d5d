"""Every attention form's backward held to the per-element rounding bounds of the plain backward (tests/test_bwd_gpu.py's (B1) and (B2)), with the bound
generalised to the forms in tests/form_ref.py: sliding window, ALiBi, softcap, attn_bias, their packed variable-length forms and the autograd functions.

Each case (form_ref.CASES; tests/test_form_bounds_cpu.py proves on the CPU that the correct algorithm fits the bound on it and that the mutants it names miss
it by 10x) runs ops.flash_attn_fwd / flash_attn_bwd or the varlen pair, takes 16-bit and fp32 gradients, and asserts
    (B1) |g32 - ref| <= b1 = eps16 * A + 1e-6      (B2) |g16 - ref| <= b1 + half an ulp16 of the result * (1 + 1e-3)      element by element,
ref = fp64 autograd of the form's definition, A = form_ref.bwd_bounds with the 16-bit O the forward stored; and exact zeros where the definition gives
zeros: dq of rows without a finite score, dk / dv of keys no row sees, every gradient of a row outside every sequence.  A packed batch is checked sequence by
sequence against fp64, the bound computed per sequence — not against another run of the kernels.  Shapes: (192,192) whole blocks only; (70,203) one ragged
block each way; (257,130) one row into the second 256-row query block; (320,385) second blocks on both sides, one key into the third 192-key block.
check_grads prints max(|d| / bound) per gradient before it asserts.
"""
import functools

import pytest
import torch

import form_ref as F

pytestmark = pytest.mark.gpu

FIXED = [c["id"] for c in F.CASES if c["kind"] == "fixed"]
VARLEN = [c["id"] for c in F.CASES if c["kind"] == "varlen"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from tiny_flash_attention_amd import _lib

    _lib.lib()
    return _lib


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """The case's tensors and, per part (the case itself, or each sequence of a packed one that has rows), the fp64 gradients and where they are exactly
    zero: computed once, shared by the ops and the autograd test of the case, never modified."""
    case = F.BY_ID[case_id] if case_id in F.BY_ID else F.sweep_case(int(case_id[len("sweep"):]))
    t = F.build(case)
    if case["kind"] == "varlen":
        parts = {b: (q, k, v, do, f) for b, q, k, v, do, f, _, _ in F.sequences(t)}
    else:
        parts = {None: (t["q"], t["k"], t["v"], t["dout"], t["form"])}
    refs = {}
    for b, (q, k, v, do, f) in parts.items():
        if k.shape[2]:
            refs[b] = (F.ref_grads(q, k, v, do, t["sc"], **f), F.structure(q, k, t["sc"], **f))
    return t, parts, refs


def form_kwargs(t, dev):
    c = t["case"]
    kw = dict(window_size=c["window"], softcap=c["cap"], alibi_slopes=None if t["slopes"] is None else t["slopes"].to(dev))
    if t["bias"] is not None:
        kw["attn_bias"] = F.bias_to_device(t["bias"], c["bias"], dev)
    return kw


def check_part(label, g32, g16, out16, part, ref, sc, dtype):
    """One (1|B, H, n, D) problem: (B1) / (B2) element by element, and the exact zeros."""
    q, k, v, do, f = part
    grads, (empty, unseen) = ref
    F.check_grads(g32, g16, grads, F.bwd_bounds(q, k, v, out16, do, sc, **f), dtype, label)
    # for the record only (profiles/forms_bwd_bounds.txt): dk against oracle.attn_bwd_bounds' Ak, which lacks the dK/dV launch's second rounding
    ak = F.bwd_bounds(q, k, v, out16, do, sc, kv_p16=False, **f)[1:2]
    print(f"{label} dk / bound without the second rounding: " + "  ".join(f"{n} {F.ratios(g[1:2], grads[1:2], ak, dtype, half_ulp=h)[0]:.3f}"
                                                                         for n, g, h in (("fp32", g32, False), ("16-bit", g16, True)) if g is not None))
    for gs in (g for g in (g32, g16) if g is not None):
        dq, dk, dv = (g.cpu() for g in gs)
        assert bool((dq[empty.unsqueeze(-1).expand_as(dq)] == 0).all()), f"{label}: dq of a row without a finite score must be exactly 0"
        for g, n in ((dk, "dk"), (dv, "dv")):
            assert bool((g[unseen.unsqueeze(-1).expand_as(g)] == 0).all()), f"{label}: {n} of a key no row sees must be exactly 0"


def run_fixed(case_id, dev):
    from tiny_flash_attention_amd import ops

    t, parts, refs = reference(case_id)
    c, sc = t["case"], t["sc"]
    q, k, v, do = (t[n].to(dev) for n in ("q", "k", "v", "dout"))
    kw = form_kwargs(t, dev)
    o, l = ops.flash_attn_fwd(q, k, v, c["causal"], sc, **kw)
    g16 = ops.flash_attn_bwd(q, k, v, o, l, do, c["causal"], sc, **kw)
    g32 = ops.flash_attn_bwd(q, k, v, o, l, do, c["causal"], sc, grad_f32=True, **kw)
    torch.cuda.synchronize()
    check_part(case_id, g32, g16, o.cpu(), parts[None], refs[None], sc, t["dtype"])


def check_packed(case_id, t, parts, refs, o, g32, g16):
    """A packed result sequence by sequence against fp64; sequences without rows or without keys and the rows outside every sequence: exact zeros."""
    cq, ck, sc = t["cu_q"], t["cu_k"], t["sc"]
    o = o.cpu()
    g32 = None if g32 is None else [g.cpu() for g in g32]
    g16 = [g.cpu() for g in g16]
    for b in range(t["B"]):
        sl = lambda gs: None if gs is None else (F.seq_view(gs[0], cq, b), F.seq_view(gs[1], ck, b), F.seq_view(gs[2], ck, b))   # noqa: E731
        if b in refs:
            check_part(f"{case_id}[seq {b}: {int(cq[b + 1] - cq[b])}x{int(ck[b + 1] - ck[b])}]", sl(g32), sl(g16), F.seq_view(o, cq, b), parts[b], refs[b], sc, t["dtype"])
        else:                                              # no query row, or no key: nothing flows
            for gs in (g for g in (sl(g32), sl(g16)) if g is not None):
                assert all(bool((g == 0).all()) for g in gs), f"{case_id}[seq {b}]: a sequence without rows or without keys has zero gradients"
    for gs in (g for g in (g32, g16) if g is not None):
        for g, n in zip(gs, (int(cq[-1]), int(ck[-1]), int(ck[-1]))):
            assert g.shape[0] > n and bool((g[n:] == 0).all()), f"{case_id}: rows outside every sequence must have exactly zero gradients"


def varlen_args(t, dev):
    c = t["case"]
    kw = form_kwargs(t, dev)
    return (t["cu_q"].to(dev), t["cu_k"].to(dev), max(1, max(c["lq"])), max(1, max(c["lk"]))), kw


def run_varlen(case_id, dev):
    from tiny_flash_attention_amd import ops

    t, parts, refs = reference(case_id)
    c, sc = t["case"], t["sc"]
    q, k, v, do = (t[n].to(dev) for n in ("q", "k", "v", "dout"))
    cu, kw = varlen_args(t, dev)
    o, l = ops.flash_attn_varlen_fwd(q, k, v, *cu, c["causal"], sc, out=torch.zeros_like(q), **kw)
    g16 = ops.flash_attn_varlen_bwd(q, k, v, o, l, do, *cu, c["causal"], sc, **kw)
    g32 = ops.flash_attn_varlen_bwd(q, k, v, o, l, do, *cu, c["causal"], sc, grad_f32=True, **kw)
    torch.cuda.synchronize()
    check_packed(case_id, t, parts, refs, o, g32, g16)


@pytest.mark.parametrize("case_id", FIXED)
def test_fixed_vs_fp64_bounds(lib, dev, case_id):
    run_fixed(case_id, dev)


@pytest.mark.parametrize("case_id", VARLEN)
def test_varlen_vs_fp64_bounds(lib, dev, case_id):
    run_varlen(case_id, dev)


@pytest.mark.parametrize("case_id", F.AUTOGRAD_IDS)
def test_autograd_vs_fp64_bounds(lib, dev, case_id):
    """flash_attn_func / flash_attn_varlen_func under autograd: q.grad, k.grad and v.grad held to (B2)."""
    import tiny_flash_attention_amd as tfa

    t, parts, refs = reference(case_id)
    c, sc = t["case"], t["sc"]
    kw = form_kwargs(t, dev)
    if c["kind"] == "varlen":
        q, k, v = (t[n].to(dev).requires_grad_(True) for n in ("q", "k", "v"))
        cu, _ = varlen_args(t, dev)
        out = tfa.flash_attn_varlen_func(q, k, v, *cu, causal=c["causal"], **kw)
        out.backward(t["dout"].to(dev))
        torch.cuda.synchronize()
        o = out.detach().clone()
        o[int(t["cu_q"][-1]):] = 0                         # (rows outside every sequence are not written)
        check_packed(case_id + "[autograd]", t, parts, refs, o, None, (q.grad, k.grad, v.grad))
    else:
        q, k, v = (t[n].to(dev).transpose(1, 2).contiguous().requires_grad_(True) for n in ("q", "k", "v"))        # (B, N, H, D)
        out = tfa.flash_attn_func(q, k, v, causal=c["causal"], **kw)
        out.backward(t["dout"].to(dev).transpose(1, 2))
        torch.cuda.synchronize()
        g16 = tuple(x.grad.transpose(1, 2) for x in (q, k, v))
        check_part(case_id + "[autograd]", None, g16, out.detach().transpose(1, 2).cpu(), parts[None], refs[None], sc, t["dtype"])


@pytest.mark.parametrize("seed", range(48))
def test_seeded_sweep(lib, dev, seed):
    case = F.sweep_case(seed)
    print({k: v for k, v in case.items() if k not in ("mutants", "na")})
    (run_varlen if case["kind"] == "varlen" else run_fixed)(case["id"], dev)
