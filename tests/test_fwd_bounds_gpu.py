"""The prefill forward family held to per-element bounds on out and on the LSE (tests/fwd_ref.py): tfa_fwd by kernel variant, the local / ALiBi / softcap / bias
forms, flash_attn_varlen_fwd, its paged form and flash_attn_fwd_splitkv.  Every case runs the public ops entry point three ways — 16-bit out, out_f32=True
and the LSE, of both launches (split-KV has no fp32 output: 16-bit out and the LSE) — and asserts, element by element against fp64, a packed batch sequence by sequence, never
against another run of the kernels, and with NO element exempt:
    fp32 out     |d| <= eps16 * A + 1e-6                                                      A = sum_j P_ij |v_jd|
    16-bit out   |d| <= eps16 * A + 1e-6 + half an ulp16 of the result * (1 + 1e-3)
    lse          |d| <= fwd_ref.lse_bound (a closed form in 2^-24 derived from the kernels' statements) AND the bar the suite had before, 1e-4 (the forms:
                 1e-4 * max(1, |lse|)) — the derived bound is the looser of the two where T is large: the peaked rows, steep slopes, saturated caps
    a row that sees no key: lse = +inf exactly and out = 0 exactly;  no NaN anywhere;
    rows outside every sequence of a packed batch, and the columns outside a column slice: the sentinel out was filled with, bit for bit (the LSE's
    sentinel goes through the C ABI: the public call allocates its LSE).
tests/test_fwd_bounds_cpu.py proves on the CPU that the correct algorithm fits the bounds on every case and that the mutants a case names miss one of them by
10x.  max(|d| / bound) is printed per quantity before it is asserted (profiles/fwd_bounds.txt).  The peaked cases turn "a row whose dominant key lies outside
its first 64-key tile still meets 2^-8 * A under TFA_RULE_FIRST_TILE" into an assertion, with and without the 2^40 re-base.
"""
import functools

import pytest
import torch

import form_ref as F
import fwd_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 7.25                  # exact in bf16, fp16 and fp32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from tiny_flash_attention_amd import _lib

    _lib.lib()
    yield _lib
    _lib.set_variant(-1)


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """The case's tensors, its parts and the fp64 reference of every part: computed once on the CPU, never modified."""
    t = R.build(R.case_of(case_id))
    return t, R.parts(t), R.reference(t)


def form_kwargs(t, dev):
    c = t["case"]
    kw = dict(window_size=c["window"], softcap=c["cap"], alibi_slopes=None if t["slopes"] is None else t["slopes"].to(dev))
    if t["bias"] is not None:
        kw["attn_bias"] = F.bias_to_device(t["bias"], c["bias"], dev)
    return kw


def call(t, dev, place=None):
    """The public call of a case, 16-bit and fp32 out: (out16, out32 or None, [the LSE of each launch]) on the CPU, out as (B,H,Nq,D) / packed (total_q,H,D), the
    LSEs as the call returns them.  place (paged cases): (k_pool, v_pool, block_table) on the device to use instead of copies of the case's."""
    from tiny_flash_attention_amd import ops

    c, sc = t["case"], t["sc"]
    d = lambda x: x.to(dev)      # noqa: E731
    if c["kind"] == "splitkv":
        o16, lse = ops.flash_attn_fwd_splitkv(d(t["q"]), d(t["k"]), d(t["v"]), c["causal"], sc, splits=c["splits"])
        torch.cuda.synchronize()
        return o16.cpu(), None, [lse.cpu()]
    if c["kind"] == "sliced":
        lo, hi = c["off"], c["off"] + c["D"]
        qf, kf, vf = (d(t[n + "_full"]) for n in ("q", "k", "v"))
        outs, lses = [], []
        for dt in (t["dtype"], torch.float32):
            full = torch.full(qf.shape, SENTINEL, dtype=dt, device=dev)
            _, lse = ops.flash_attn_fwd(qf[..., lo:hi], kf[..., lo:hi], vf[..., lo:hi], c["causal"], sc, out=full[..., lo:hi])
            o, l = ops.flash_attn_fwd(d(t["q"]), d(t["k"]), d(t["v"]), c["causal"], sc, out_f32=dt == torch.float32)      # the same problem, contiguous
            torch.cuda.synchronize()
            full = full.cpu()
            assert bool((full[..., :lo] == SENTINEL).all()) and bool((full[..., hi:] == SENTINEL).all()), f"{c['id']}: columns outside the slice were written"
            assert torch.equal(full[..., lo:hi], o.cpu()) and torch.equal(lse, l), f"{c['id']}: the column slice changed the result"
            outs.append(full[..., lo:hi])
            lses.append(lse.cpu())
        return outs[0], outs[1], lses
    if R.packed(c):
        cq, ck = d(t["cu_q"]), d(t["cu_k"])
        mq, mk = max(1, max(c["lq"])), max(1, max(c["lk"]))
        if c["kind"] == "paged":
            k, v, bt = (d(t["k_pool"]), d(t["v_pool"]), d(t["bt"])) if place is None else place
            kw = dict(block_table=bt)
        else:
            k, v, kw = d(t["k"]), d(t["v"]), form_kwargs(t, dev)
        q = d(t["q"])
        outs, lses = [], []
        for dt in (t["dtype"], torch.float32):
            out = torch.full(q.shape, SENTINEL, dtype=dt, device=dev)
            o, lse = ops.flash_attn_varlen_fwd(q, k, v, cq, ck, mq, mk, c["causal"], sc, out=out, **kw)
            torch.cuda.synchronize()
            n = int(t["cu_q"][-1])
            assert o.shape[0] > n and bool((o[n:] == SENTINEL).all()), f"{c['id']}: rows outside every sequence were written"
            assert tuple(lse.shape) == (c["H"], q.shape[0]) and lse.dtype == torch.float32
            outs.append(o.cpu())
            lses.append(lse.cpu())
        return outs[0], outs[1], lses
    q, k, v = d(t["q"]), d(t["k"]), d(t["v"])
    if c["layout"] == "bnhd":
        q, k, v = (x.transpose(1, 2).contiguous() for x in (q, k, v))
    kw = form_kwargs(t, dev)
    o16, lse = ops.flash_attn_fwd(q, k, v, c["causal"], sc, layout=c["layout"], **kw)
    o32, lse32 = ops.flash_attn_fwd(q, k, v, c["causal"], sc, layout=c["layout"], out_f32=True, **kw)
    torch.cuda.synchronize()
    assert o16.dtype == t["dtype"] and o32.dtype == torch.float32
    for l in (lse, lse32):
        assert tuple(l.shape) == (c["B"], c["H"], c["Nq"]) and l.dtype == torch.float32
    if c["layout"] == "bnhd":
        o16, o32 = o16.transpose(1, 2), o32.transpose(1, 2)
    return o16.cpu(), o32.cpu(), [lse.cpu(), lse32.cpu()]


def run_case(case_id, dev, lib, place=None):
    """The case against its bounds; returns what call() returned.  place: a function of the case's tensors that returns call()'s place."""
    t, parts, ref = reference(case_id)
    c, dtype = t["case"], t["dtype"]
    lib.set_variant(c["variant"])
    try:
        if c["peak"] is not None:                           # what the case is in the list for: the library says it rounds against the first tile's maximum
            rule = lib.rule_for(c["B"], c["H"], c["Hk"], c["Nq"], c["Nk"], c["D"], c["causal"], lib.TFA_BF16)
            assert rule == lib.RULE_FIRST_TILE, f"{case_id}: rounding rule {rule}, not TFA_RULE_FIRST_TILE"
        o16, o32, lses = call(t, dev, None if place is None else place(t))
    finally:
        lib.set_variant(-1)
    worst = {"out32": 0.0, "out16": 0.0, "lse": 0.0, "lse_old": 0.0}
    empty = 0
    keys = list(range(len(c["lq"]))) if R.packed(c) else [None]
    for key in keys:
        if key is None:
            g16, g32, gls = o16, o32, lses
        else:
            if c["lq"][key] == 0:
                continue
            g16, g32 = F.seq_view(o16, t["cu_q"], key), None if o32 is None else F.seq_view(o32, t["cu_q"], key)
            gls = [l[:, int(t["cu_q"][key]):int(t["cu_q"][key + 1])].unsqueeze(0) for l in lses]
        what = f"{case_id}" + ("" if key is None else f"[seq {key}: {c['lq'][key]}x{c['lk'][key]}]")
        outs = [(n, g) for n, g in (("out16", g16), ("out32", g32)) if g is not None]
        for n, g in outs:
            assert not bool(torch.isnan(g).any()), f"{what}: NaN in {n}"
        assert not any(bool(torch.isnan(gl).any()) for gl in gls), f"{what}: NaN in the LSE"
        if key not in parts:                                # rows, but no key: nothing to attend
            assert all(bool(torch.isposinf(gl).all()) for gl in gls) and all(bool((g == 0).all()) for _, g in outs), f"{what}: a sequence without keys gives out = 0, lse = +inf"
            continue
        out, l64, A, T, bound = ref[key]
        unseen = torch.isposinf(l64)
        for gl in gls:
            assert torch.equal(torch.isposinf(gl), unseen), f"{what}: lse = +inf on other rows than the definition's"
        for n, g in outs:
            assert bool((g[unseen.unsqueeze(-1).expand_as(g)] == 0).all()), f"{what}: {n} != 0 on a row that sees no key"
        empty += int(unseen.sum())
        old_bar = R.old_lse_bar(torch.where(unseen, torch.zeros_like(l64), l64), R.has_form(c))
        got = {"out16": R.out_ratio(g16.double(), out, A, dtype, True), "lse": max(R.lse_ratio(gl, l64, bound) for gl in gls),        # (the LSE of BOTH launches)
               "lse_old": max(R.lse_ratio(gl, l64, old_bar) for gl in gls)}
        if g32 is not None:
            got["out32"] = R.out_ratio(g32.double(), out, A, dtype, False)
        print(f"{what}: max(|d| / bound) " + "  ".join(f"{n} {r:.4f}" for n, r in got.items()) + f"  (largest T {T.max().item():.1f})")
        for n, r in got.items():
            worst[n] = max(worst[n], r)
    print(f"{case_id} {'bf16' if dtype == torch.bfloat16 else 'fp16'} variant {c['variant']}: max(|d| / bound) " + "  ".join(f"{n} {r:.4f}" for n, r in worst.items())
          + f"  (rows without a key: {empty})")
    assert worst["out32"] <= 1.0, f"{case_id}: the fp32 out is at {worst['out32']:.3f} of eps16 * A + 1e-6"
    assert worst["out16"] <= 1.0, f"{case_id}: the 16-bit out is at {worst['out16']:.3f} of its per-element bound"
    assert worst["lse"] <= 1.0, f"{case_id}: the LSE is at {worst['lse']:.3f} of its derived bound"
    assert worst["lse_old"] <= 1.0, f"{case_id}: the LSE is at {worst['lse_old']:.3f} of the earlier bar, 1e-4 (the forms: * max(1, |lse|))"
    return o16, o32, lses


def ids(pred):
    return [c["id"] for c in R.CASES if pred(c)]


@pytest.mark.parametrize("case_id", ids(lambda c: c["id"].startswith("plain-")))
def test_plain_by_variant(lib, dev, case_id):
    run_case(case_id, dev, lib)


@pytest.mark.parametrize("case_id", ids(lambda c: c["id"].startswith("form-") and c["kind"] == "fixed"))
def test_forms(lib, dev, case_id):
    run_case(case_id, dev, lib)


@pytest.mark.parametrize("case_id", ids(lambda c: c["kind"] == "varlen"))
def test_packed(lib, dev, case_id):
    run_case(case_id, dev, lib)


@pytest.mark.parametrize("case_id", ["varlen-d128-bf16-c-v30", "varlen-d40-bf16-f-vauto"])
def test_packed_lse_sentinel(lib, dev, case_id):
    """ops.flash_attn_varlen_fwd allocates its LSE, so the sentinel there goes through the C ABI (tfa_fwd_varlen with a caller-owned lse): the columns of the rows
    outside every sequence keep it bit for bit, the others are the public call's bits."""
    import ctypes as C

    from tiny_flash_attention_amd import ops

    t, _, _ = reference(case_id)
    c = t["case"]
    q, k, v, cq, ck = (t[n].to(dev) for n in ("q", "k", "v", "cu_q", "cu_k"))
    mq, mk = max(c["lq"]), max(c["lk"])
    out = torch.full(q.shape, SENTINEL, dtype=q.dtype, device=dev)
    lse = torch.full((c["H"], q.shape[0]), SENTINEL, dtype=torch.float32, device=dev)
    p = lib.TfaVarlenFwdParams()
    p.q, p.k, p.v, p.out, p.lse = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr()
    p.cu_seqlens_q, p.cu_seqlens_k = cq.data_ptr(), ck.data_ptr()
    p.B, p.H, p.Hk, p.D = len(c["lq"]), c["H"], c["Hk"], c["D"]
    p.max_seqlen_q, p.max_seqlen_k, p.total_q, p.total_k = mq, mk, q.shape[0], k.shape[0]
    for name, x in (("q_stride", q), ("k_stride", k), ("v_stride", v), ("o_stride", out)):
        arr = getattr(p, name)
        arr[0], arr[1] = x.stride(1), x.stride(0)
    p.softmax_scale, p.is_causal = t["sc"], int(c["causal"])
    p.dtype = p.out_dtype = lib.TFA_BF16 if q.dtype == torch.bfloat16 else lib.TFA_F16
    lib.set_variant(c["variant"])
    try:
        with torch.cuda.device(dev):
            lib.check(lib.lib().tfa_fwd_varlen(C.byref(p), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        o2, l2 = ops.flash_attn_varlen_fwd(q, k, v, cq, ck, mq, mk, c["causal"], t["sc"])
        torch.cuda.synchronize()
    finally:
        lib.set_variant(-1)
    n = int(t["cu_q"][-1])
    assert lse.shape[1] > n and bool((lse[:, n:] == SENTINEL).all()) and bool((out[n:] == SENTINEL).all()), "rows outside every sequence were written"
    assert torch.equal(lse[:, :n], l2[:, :n]) and torch.equal(out[:n], o2[:n])


@pytest.mark.parametrize("case_id", ids(lambda c: c["kind"] == "paged"))
def test_paged(lib, dev, case_id):
    run_case(case_id, dev, lib)


@pytest.mark.parametrize("case_id", ids(lambda c: c["kind"] == "splitkv"))
def test_splitkv(lib, dev, case_id):
    run_case(case_id, dev, lib)


@pytest.mark.parametrize("case_id", ids(lambda c: c["peak"] is not None))
def test_peaked_rows(lib, dev, case_id):
    run_case(case_id, dev, lib)


@pytest.mark.parametrize("case_id", ids(lambda c: c["kind"] == "sliced"))
def test_strided_slice(lib, dev, case_id):
    run_case(case_id, dev, lib)


@pytest.mark.parametrize("seed", range(48))
def test_seeded_sweep(lib, dev, seed):
    case = R.sweep_case(seed)
    print({k: v for k, v in case.items() if k not in ("mutants", "na")})
    run_case(case["id"], dev, lib)
