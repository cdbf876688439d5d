"""GPU tests of the packed variable-length forward and backward (include/tfa.h: tfa_fwd_varlen, tfa_bwd_varlen; ops.flash_attn_varlen_*).

  1. equal lengths are bit-identical to the fixed-length path (same kernel, forced to the varlen call's variant where the fixed dispatch picks a key-split one);
  2. mixed lengths against the fp64 oracle per sequence, with the header's bars: atol 1e-2 on 16-bit out, eps16 * A + 1e-6 on fp32 out, LSE within 1e-4
     and +inf exactly where a row sees no key, and the same-rounding-points bound 1e-3 |ref| + 1e-4 A against the emulation of the reported rule;
     — on the kernel the sizes pick (il4 here) and on il8 (variant 30) forced, both dtypes, both widths, fp32 and 16-bit out;
  3. isolation: rows past cu[B] (NaN) are never read into a result, out / lse rows outside every sequence are never written (il4 and il8), nor are
     dq / dk / dv rows by tfa_bwd_varlen itself;
  4. backward against fp64 per sequence: the (B1)/(B2)/(B3) bounds of test_bwd_gpu.py, GQA sums, determinism;
  5. autograd: flash_attn_varlen_func against per-sequence flash_attn_func, zero gradients on padding rows;
  6. graph capture with cu_seqlens in static device buffers: new lengths, one replay, equal to an eager call (no host read of cu_seqlens).
"""
import ctypes as C
import math

import pytest
import torch

from helpers import ulp16

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tfa():
    import tiny_flash_attention_amd as m
    from tiny_flash_attention_amd import _lib

    _lib.lib()
    return m


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O

    return O


def rnd(shape, dtype, seed, std=0.5):
    g = torch.Generator().manual_seed(seed)
    return torch.empty(shape, dtype=torch.float32).normal_(0.0, std, generator=g).to(dtype)


def cu_of(lens):
    c = [0]
    for n in lens:
        c.append(c[-1] + n)
    return torch.tensor(c, dtype=torch.int32)


def varlen_variant(B, H, Hk, D, max_q, max_k, total_q, total_k, causal, dtype):
    from tiny_flash_attention_amd import _lib

    p = _lib.TfaVarlenFwdParams()
    p.q = p.k = p.v = p.out = p.lse = p.cu_seqlens_q = p.cu_seqlens_k = 0x10000
    p.B, p.H, p.Hk, p.D = B, H, Hk, D
    p.max_seqlen_q, p.max_seqlen_k, p.total_q, p.total_k = max_q, max_k, total_q, total_k
    for name, h in (("q_stride", H), ("k_stride", Hk), ("v_stride", Hk), ("o_stride", H)):
        getattr(p, name)[0], getattr(p, name)[1] = D, h * D
    p.softmax_scale, p.is_causal = 1.0, int(causal)
    p.dtype = p.out_dtype = _lib.TFA_BF16 if dtype == torch.bfloat16 else _lib.TFA_F16
    L = _lib.lib()
    v, r = L.tfa_fwd_varlen_variant(C.byref(p)), L.tfa_fwd_varlen_rounding_rule(C.byref(p))
    assert v in (30, 32) and r in (_lib.RULE_LAZY, _lib.RULE_FIRST_TILE)
    return v, r


class forced:
    """run the block with the calling thread's kernel variant forced (tfa_set_variant; None = automatic).  The small problems of these tests all pick il4
    (variant 32) by themselves; il8 (30) — what packed batches at realistic sizes run, with its own first-pass Q through LDS (QLDS) and the next pass's
    requests issued from the epilogue (PREF2) — is forced here so that its varlen instantiations see ragged, empty and Nq != Nk sequences too."""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        from tiny_flash_attention_amd import _lib

        if self.v is not None:
            _lib.set_variant(self.v)

    def __exit__(self, *exc):
        from tiny_flash_attention_amd import _lib

        _lib.set_variant(-1)
        return False


def seq(t, cu, b):
    """rows of sequence b of a packed (total, heads, D) tensor as a (1, heads, n, D) CPU tensor"""
    return t[int(cu[b]):int(cu[b + 1])].cpu().permute(1, 0, 2).unsqueeze(0)


# ---- 1. equal lengths: bit-identical to the fixed-length path ------------------------------------------------------------------

EQUAL = [  # (B, H, Hk, N, D, dtype)
    (4, 32, 32, 4096, 128, torch.bfloat16),
    (4, 8, 8, 1024, 64, torch.float16),
    (4, 32, 8, 4096, 128, torch.bfloat16),
]


@pytest.mark.parametrize("B,H,Hk,N,D,dtype", EQUAL)
@pytest.mark.parametrize("causal", [True, False])
def test_equal_lengths_bit_identical(tfa, dev, B, H, Hk, N, D, dtype, causal):
    from tiny_flash_attention_amd import _lib, ops

    sc = 1.0 / math.sqrt(D)
    q4 = rnd((B, N, H, D), dtype, 1).to(dev)
    k4 = rnd((B, N, Hk, D), dtype, 2).to(dev)
    v4 = rnd((B, N, Hk, D), dtype, 3).to(dev)
    do4 = rnd((B, N, H, D), dtype, 4).to(dev)
    cu = cu_of([N] * B).to(dev)
    var, _ = varlen_variant(B, H, Hk, D, N, N, B * N, B * N, causal, dtype)
    fixed_var = _lib.variant_for(B, H, Hk, N, N, D, causal)
    assert var == (32 if fixed_var in (36, 37) else fixed_var)
    q, k, v, do = (t.reshape(B * N, t.shape[2], D) for t in (q4, k4, v4, do4))
    out, lse = ops.flash_attn_varlen_fwd(q, k, v, cu, cu, N, N, causal, sc)
    dq, dk, dv = ops.flash_attn_varlen_bwd(q, k, v, out, lse, do, cu, cu, N, N, causal, sc)
    _lib.set_variant(var)                              # (the fixed dispatch's key-split choice: forced to the kernel the varlen call ran)
    try:
        out4, lse4 = ops.flash_attn_fwd(q4, k4, v4, causal, sc, layout="bnhd")
    finally:
        _lib.set_variant(-1)
    g4 = ops.flash_attn_bwd(q4, k4, v4, out4, lse4, do4, causal, sc, layout="bnhd")
    torch.cuda.synchronize()
    assert torch.equal(out.view(B, N, H, D), out4)
    assert torch.equal(lse, lse4.permute(1, 0, 2).reshape(H, B * N))
    for name, a, b4 in zip(("dq", "dk", "dv"), (dq, dk, dv), g4):
        assert torch.equal(a.view(b4.shape), b4), name


# ---- 2. mixed lengths against the fp64 oracle ----------------------------------------------------------------------------------

MIX_LONG = ([0, 1, 63, 64, 65, 255, 256, 257, 1000, 3000, 10],
            [5, 1, 63, 100, 65, 255, 300, 200, 1000, 3000, 0])         # Nq > Nk (65/65 equal, 257 > 200, 10 > 0), Nq < Nk, empty ones
MIX_SHORT = ([0, 1, 63, 64, 65, 255, 256, 257, 700, 7],
             [9, 1, 63, 100, 40, 255, 300, 200, 1000, 0])

MIXED = [  # (D, dtype, H, Hk, causal, mix, forced variant)
    (128, torch.bfloat16, 2, 2, True, MIX_LONG, None),
    (128, torch.float16, 4, 2, False, MIX_SHORT, None),
    (64, torch.float16, 2, 2, True, MIX_LONG, None),
    (64, torch.bfloat16, 4, 1, True, MIX_SHORT, None),
    (96, torch.bfloat16, 2, 2, True, MIX_SHORT, None),
    (40, torch.float16, 4, 2, True, MIX_SHORT, None),
    (8, torch.bfloat16, 2, 2, False, MIX_SHORT, None),
    (8, torch.float16, 2, 1, True, MIX_SHORT, None),
    # il8 (variant 30): both dtypes, both kernel widths, causal (paired blocks: 700 rows = three 256-row blocks, an odd count) and not, GQA
    (128, torch.bfloat16, 2, 2, True, MIX_LONG, 30),
    (128, torch.float16, 2, 2, True, MIX_SHORT, 30),
    (128, torch.bfloat16, 4, 2, False, MIX_SHORT, 30),
    (64, torch.float16, 2, 2, True, MIX_LONG, 30),
    (64, torch.bfloat16, 4, 1, True, MIX_SHORT, 30),
    (64, torch.float16, 4, 2, False, MIX_SHORT, 30),
]


def emulate(oracle, rule, bm, q, k, v, causal, sc):
    from tiny_flash_attention_amd import _lib

    if rule == _lib.RULE_FIRST_TILE:
        return oracle.tiled_emulation_first_tile(q, k, v, causal, sc, 64, block_m=bm, return_lse=True)
    return oracle.tiled_emulation_lazy(q, k, v, causal, sc, 64, return_lse=True)


@pytest.mark.parametrize("D,dtype,H,Hk,causal,mix,force", MIXED)
def test_mixed_lengths_against_fp64(tfa, oracle, dev, D, dtype, H, Hk, causal, mix, force):
    from tiny_flash_attention_amd import ops

    lq, lk = mix
    B = len(lq)
    cq, ck = cu_of(lq), cu_of(lk)
    tq, tk = int(cq[-1]), int(ck[-1])
    sc = 1.0 / math.sqrt(D)
    q = rnd((tq, H, D), dtype, 11).to(dev)
    k = rnd((tk, Hk, D), dtype, 12).to(dev)
    v = rnd((tk, Hk, D), dtype, 13).to(dev)
    with forced(force):
        var, rule = varlen_variant(B, H, Hk, D, max(lq), max(lk), tq, tk, causal, dtype)
        o16, lse = ops.flash_attn_varlen_fwd(q, k, v, cq.to(dev), ck.to(dev), max(lq), max(lk), causal, sc)
        o32, _ = ops.flash_attn_varlen_fwd(q, k, v, cq.to(dev), ck.to(dev), max(lq), max(lk), causal, sc, out_f32=True)
    torch.cuda.synchronize()
    assert force is None or var == force
    bm = 256 if var == 30 else 128
    eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    for b in range(B):
        nq, nk = lq[b], lk[b]
        if nq == 0:
            continue
        qb, kb, vb = seq(q, cq, b), seq(k, ck, b), seq(v, ck, b)
        a16, a32 = seq(o16, cq, b).float(), seq(o32, cq, b)
        lb = lse[:, int(cq[b]):int(cq[b + 1])].cpu().unsqueeze(0)
        assert bool(torch.isfinite(a16).all()) and bool(torch.isfinite(a32).all()), f"seq {b}"
        if nk == 0:
            assert bool((a16 == 0).all()) and bool((a32 == 0).all()) and bool(torch.isinf(lb).all() and (lb > 0).all()), f"seq {b}: no keys"
            continue
        exact, lse_x = oracle.exact64(qb, kb, vb, causal, sc, return_lse=True)
        A = oracle.abs_weighted(qb, kb, vb, causal, sc)
        d16 = (a16.double() - exact).abs().max().item()
        assert d16 <= 1e-2, f"seq {b} ({nq}x{nk}): 16-bit out max|d| = {d16:.3e}"
        assert bool(((a32.double() - exact).abs() <= eps * A + 1e-6).all()), f"seq {b}: fp32 out beyond the P-rounding bound"
        empty = torch.isinf(lse_x)
        assert torch.equal(torch.isinf(lb) & (lb > 0), empty), f"seq {b}: +inf LSE exactly where a row sees no key"
        assert (lb[~empty].double() - lse_x[~empty]).abs().max().item() <= 1e-4 if bool((~empty).any()) else True, f"seq {b}: LSE"
        emu, _ = emulate(oracle, rule, bm, qb, kb, vb, causal, sc)
        viol = ((a32 - emu).abs() > 1e-3 * emu.abs() + 1e-4 * A.float()).float().mean().item()
        assert viol <= 1e-4, f"seq {b}: {viol:.2e} of elements beyond the same-rounding-points bound"


# ---- 3. isolation ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,dtype,causal", [(128, torch.bfloat16, True), (64, torch.float16, False), (128, torch.float16, True), (64, torch.bfloat16, True)])
@pytest.mark.parametrize("force", [None, 30])
def test_padding_rows_isolated(tfa, dev, D, dtype, causal, force):
    from tiny_flash_attention_amd import ops

    lq, lk = [100, 0, 257, 31], [64, 77, 300, 0]
    pad_q, pad_k = 45, 70
    H, Hk = 4, 2
    cq, ck = cu_of(lq), cu_of(lk)
    tq, tk = int(cq[-1]) + pad_q, int(ck[-1]) + pad_k
    q = rnd((tq, H, D), dtype, 21)
    k = rnd((tk, Hk, D), dtype, 22)
    v = rnd((tk, Hk, D), dtype, 23)
    q[int(cq[-1]):] = float("nan")
    k[int(ck[-1]):] = float("nan")
    v[int(ck[-1]):] = float("nan")
    q, k, v = q.to(dev), k.to(dev), v.to(dev)
    for f32 in (False, True):
        out = torch.full((tq, H, D), 7.5, dtype=torch.float32 if f32 else dtype, device=dev)
        ref_out = out.clone()
        with forced(force):
            out, lse = ops.flash_attn_varlen_fwd(q, k, v, cq.to(dev), ck.to(dev), max(lq), max(lk), causal, None, out=out)
        torch.cuda.synchronize()
        n = int(cq[-1])
        assert bool(torch.isfinite(out[:n]).all()) and not bool(torch.isnan(lse[:, :n]).any())
        assert torch.equal(out[n:], ref_out[n:]), "out rows outside every sequence were written"
    # lse rows outside every sequence: a sentinel-filled buffer through the C ABI's own lse pointer
    from tiny_flash_attention_amd import _lib
    lse_s = torch.full((H, tq), -3.25, dtype=torch.float32, device=dev)
    out = torch.empty((tq, H, D), dtype=dtype, device=dev)
    p = _lib.TfaVarlenFwdParams()
    p.q, p.k, p.v, p.out, p.lse = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse_s.data_ptr()
    cqd, ckd = cq.to(dev), ck.to(dev)
    p.cu_seqlens_q, p.cu_seqlens_k = cqd.data_ptr(), ckd.data_ptr()
    p.B, p.H, p.Hk, p.D = len(lq), H, Hk, D
    p.max_seqlen_q, p.max_seqlen_k, p.total_q, p.total_k = max(lq), max(lk), tq, tk
    for name, t in (("q_stride", q), ("k_stride", k), ("v_stride", v), ("o_stride", out)):
        getattr(p, name)[0], getattr(p, name)[1] = t.stride(1), t.stride(0)
    p.softmax_scale, p.is_causal = 1.0 / math.sqrt(D), int(causal)
    p.dtype = p.out_dtype = _lib.TFA_BF16 if dtype == torch.bfloat16 else _lib.TFA_F16
    with forced(force):
        assert force is None or _lib.lib().tfa_fwd_varlen_variant(C.byref(p)) == force
        _lib.check(_lib.lib().tfa_fwd_varlen(C.byref(p), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    n = int(cq[-1])
    assert bool((lse_s[:, n:] == -3.25).all()), "lse rows outside every sequence were written"
    assert not bool(torch.isnan(lse_s[:, :n]).any())


@pytest.mark.parametrize("D,dtype,causal", [(128, torch.bfloat16, True), (64, torch.float16, False)])
@pytest.mark.parametrize("grad_f32", [False, True])
def test_backward_padding_rows_not_written(tfa, dev, D, dtype, causal, grad_f32):
    """tfa_bwd_varlen itself (not the Python wrapper, which zero-fills): dq / dk / dv rows outside every sequence keep a sentinel, rows inside are finite."""
    from tiny_flash_attention_amd import _lib, ops

    lq, lk = [100, 0, 257, 31], [64, 77, 300, 0]
    pad_q, pad_k = 45, 70
    H, Hk = 4, 2
    cq, ck = cu_of(lq), cu_of(lk)
    nq, nk = int(cq[-1]), int(ck[-1])
    tq, tk = nq + pad_q, nk + pad_k
    sc = 1.0 / math.sqrt(D)
    q, do = rnd((tq, H, D), dtype, 61), rnd((tq, H, D), dtype, 64)
    k, v = rnd((tk, Hk, D), dtype, 62), rnd((tk, Hk, D), dtype, 63)
    for t, n in ((q, nq), (do, nq), (k, nk), (v, nk)):
        t[n:] = float("nan")
    q, k, v, do = q.to(dev), k.to(dev), v.to(dev), do.to(dev)
    cqd, ckd = cq.to(dev), ck.to(dev)
    out, lse = ops.flash_attn_varlen_fwd(q, k, v, cqd, ckd, max(lq), max(lk), causal, sc)
    gdt = torch.float32 if grad_f32 else dtype
    dq = torch.full((tq, H, D), -5.5, dtype=gdt, device=dev)
    dk = torch.full((tk, Hk, D), -5.5, dtype=gdt, device=dev)
    dv = torch.full((tk, Hk, D), -5.5, dtype=gdt, device=dev)
    delta = torch.empty((H, tq), dtype=torch.float32, device=dev)
    p = _lib.TfaVarlenBwdParams()
    p.q, p.k, p.v, p.out, p.dout = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), do.data_ptr()
    p.lse, p.delta, p.dq, p.dk, p.dv = lse.data_ptr(), delta.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    p.cu_seqlens_q, p.cu_seqlens_k = cqd.data_ptr(), ckd.data_ptr()
    p.B, p.H, p.Hk, p.D = len(lq), H, Hk, D
    p.max_seqlen_q, p.max_seqlen_k, p.total_q, p.total_k = max(lq), max(lk), tq, tk
    for name, t in (("q_stride", q), ("k_stride", k), ("v_stride", v), ("o_stride", out), ("do_stride", do),
                    ("dq_stride", dq), ("dk_stride", dk), ("dv_stride", dv)):
        getattr(p, name)[0], getattr(p, name)[1] = t.stride(1), t.stride(0)
    p.softmax_scale, p.is_causal = sc, int(causal)
    p.dtype = _lib.TFA_BF16 if dtype == torch.bfloat16 else _lib.TFA_F16
    p.grad_dtype = _lib.TFA_F32 if grad_f32 else p.dtype
    _lib.check(_lib.lib().tfa_bwd_varlen(C.byref(p), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    for name, g, n in (("dq", dq, nq), ("dk", dk, nk), ("dv", dv, nk)):
        assert bool((g[n:] == -5.5).all()), f"{name} rows outside every sequence were written"
        assert bool(torch.isfinite(g[:n]).all()), f"{name}: non-finite inside the sequences"


# ---- 4. backward against fp64 ------------------------------------------------------------------------------------------------

BWD = [  # (D, dtype, H, Hk, causal, mix)
    (128, torch.bfloat16, 2, 2, True, MIX_SHORT),
    (128, torch.float16, 4, 2, False, MIX_SHORT),
    (64, torch.bfloat16, 4, 1, True, MIX_SHORT),
    (64, torch.float16, 2, 2, True, MIX_SHORT),
    (40, torch.bfloat16, 2, 2, True, MIX_SHORT),
    (96, torch.float16, 4, 2, True, MIX_SHORT),
]


@pytest.mark.parametrize("D,dtype,H,Hk,causal,mix", BWD)
def test_backward_against_fp64(tfa, oracle, dev, D, dtype, H, Hk, causal, mix):
    """Per sequence: the (B1)/(B2)/(B3) bounds of test_bwd_gpu.py against the fp64 oracle, and the fixed-length tfa_bwd on the sequence alone (same
    out / lse): bit-identical where it runs the same instantiation (head dims that fill the kernel's last 32-column block).  The bounds are the fixed-length
    kernels' own: a sequence whose fp32 gradient misses (B1) must be one where tfa_bwd gives the very same bits (measured: 256 x 300 keys, bf16, D128,
    causal — dk beyond eps16 * A + 1e-6 by 4.9e-7 on both paths)."""
    from tiny_flash_attention_amd import ops

    lq, lk = mix
    B = len(lq)
    cq, ck = cu_of(lq), cu_of(lk)
    tq, tk = int(cq[-1]), int(ck[-1])
    sc = 1.0 / math.sqrt(D)
    q = rnd((tq, H, D), dtype, 31).to(dev)
    k = rnd((tk, Hk, D), dtype, 32).to(dev)
    v = rnd((tk, Hk, D), dtype, 33).to(dev)
    do = rnd((tq, H, D), dtype, 34).to(dev)
    cqd, ckd = cq.to(dev), ck.to(dev)
    out, lse = ops.flash_attn_varlen_fwd(q, k, v, cqd, ckd, max(lq), max(lk), causal, sc)
    g16 = ops.flash_attn_varlen_bwd(q, k, v, out, lse, do, cqd, ckd, max(lq), max(lk), causal, sc)
    g16b = ops.flash_attn_varlen_bwd(q, k, v, out, lse, do, cqd, ckd, max(lq), max(lk), causal, sc)
    g32 = ops.flash_attn_varlen_bwd(q, k, v, out, lse, do, cqd, ckd, max(lq), max(lk), causal, sc, grad_f32=True)
    torch.cuda.synchronize()
    for a, b_ in zip(g16, g16b):
        assert torch.equal(a, b_), "backward is not deterministic"
    same_inst = D % 64 == 0 or D % 64 > 32          # the fixed-length launches' narrow instantiations start at 32 empty columns
    eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    for b in range(B):
        nq, nk = lq[b], lk[b]
        cur = (cq, ck, ck)
        if nq == 0 or nk == 0:                          # nothing to attend: every gradient of the sequence is zero
            for name, g, c in zip(("dq", "dk", "dv"), g16, cur):
                assert bool((seq(g, c, b) == 0).all()), f"seq {b} {name}: empty sequence, nonzero gradient"
            continue
        sl_q, sl_k = slice(int(cq[b]), int(cq[b + 1])), slice(int(ck[b]), int(ck[b + 1]))
        fixed32 = ops.flash_attn_bwd(q[sl_q][None], k[sl_k][None], v[sl_k][None], out[sl_q][None], lse[:, sl_q][None].contiguous(), do[sl_q][None],
                                     causal, sc, layout="bnhd", grad_f32=True)
        qb, kb, vb, dob, ob = seq(q, cq, b), seq(k, ck, b), seq(v, ck, b), seq(do, cq, b), seq(out, cq, b)
        ref = oracle.attn_bwd_reference(qb, kb, vb, dob, causal, sc)
        bounds = oracle.attn_bwd_bounds(qb, kb, vb, ob, dob, causal, sc)
        for i, (name, r, A) in enumerate(zip(("dq", "dk", "dv"), ref, bounds)):
            c = cur[i]
            a32, a16 = seq(g32[i], c, b).double(), seq(g16[i], c, b).double()
            f32 = fixed32[i].cpu().permute(0, 2, 1, 3).double()
            if same_inst:
                assert torch.equal(a32, f32), f"seq {b} ({nq}x{nk}) {name}: differs from tfa_bwd on the sequence alone"
            assert bool(torch.isfinite(a16).all()), f"seq {b} {name}: non-finite"
            ex = ((a32 - r).abs() - (eps * A + 1e-6)).max().item()
            assert ex <= 0 or (same_inst and torch.equal(a32, f32)), f"(B1) seq {b} ({nq}x{nk}) {name}: exceeds the 16-bit rounding bound by {ex:.3e}"
            # (B2: half an ulp of the value that was ROUNDED — the fp32 result — or of the reference, whichever binade is higher)
            ulp = ulp16(torch.maximum(r.abs(), a32.abs()).float(), dtype).double()
            ex16 = ((a16 - r).abs() - (max(ex, 0.0) + eps * A + 0.5 * ulp * (1 + 1e-3) + 1e-6)).max().item()
            assert ex16 <= 0, f"(B2) seq {b} {name}: exceeds bound + half an ulp by {ex16:.3e}"
            assert (a16 - r).abs().max().item() <= 1e-2 * max(1.0, r.abs().max().item()), f"(B3) seq {b} {name}"


# ---- 5. autograd -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,D,H,Hk,causal", [(torch.bfloat16, 128, 4, 2, True), (torch.float16, 64, 2, 2, False)])
def test_autograd_against_per_sequence(tfa, oracle, dev, dtype, D, H, Hk, causal):
    lq, lk = [100, 257, 31, 64], [64, 300, 31, 129]
    pad = 19
    cq, ck = cu_of(lq), cu_of(lk)
    tq, tk = int(cq[-1]) + pad, int(ck[-1]) + pad
    sc = 1.0 / math.sqrt(D)
    q = rnd((tq, H, D), dtype, 41).to(dev).requires_grad_(True)
    k = rnd((tk, Hk, D), dtype, 42).to(dev).requires_grad_(True)
    v = rnd((tk, Hk, D), dtype, 43).to(dev).requires_grad_(True)
    do = rnd((tq, H, D), dtype, 44).to(dev)
    out = tfa.flash_attn_varlen_func(q, k, v, cq.to(dev), ck.to(dev), max(lq), max(lk), 0.0, sc, causal)
    out.backward(do)
    eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    assert bool((q.grad[int(cq[-1]):] == 0).all()) and bool((k.grad[int(ck[-1]):] == 0).all()) and bool((v.grad[int(ck[-1]):] == 0).all())
    for b in range(len(lq)):
        sl_q, sl_k = slice(int(cq[b]), int(cq[b + 1])), slice(int(ck[b]), int(ck[b + 1]))
        qs = q.detach()[sl_q].unsqueeze(0).clone().requires_grad_(True)
        ks = k.detach()[sl_k].unsqueeze(0).clone().requires_grad_(True)
        vs = v.detach()[sl_k].unsqueeze(0).clone().requires_grad_(True)
        os_ = tfa.flash_attn_func(qs, ks, vs, causal, sc)
        os_.backward(do[sl_q].unsqueeze(0))
        assert (os_[0].float() - out.detach()[sl_q].float()).abs().max().item() <= 1e-2
        qb, kb, vb, dob = (t.detach().cpu().permute(0, 2, 1, 3) for t in (qs, ks, vs, do[sl_q].unsqueeze(0)))
        ref = oracle.attn_bwd_reference(qb, kb, vb, dob, causal, sc)
        bounds = oracle.attn_bwd_bounds(qb, kb, vb, os_.detach().cpu().permute(0, 2, 1, 3), dob, causal, sc)
        for name, gv, gf, r, A, sl in zip(("dq", "dk", "dv"), (q.grad, k.grad, v.grad), (qs.grad, ks.grad, vs.grad), ref, bounds, (sl_q, sl_k, sl_k)):
            a = gv[sl].cpu().permute(1, 0, 2).unsqueeze(0).double()
            f = gf.cpu().permute(0, 2, 1, 3).double()
            bound = eps * A + 0.5 * ulp16(torch.maximum(r.abs(), torch.maximum(a.abs(), f.abs())).float(), dtype).double() * (1 + 1e-3) + 1e-6
            assert ((a - r).abs() - bound).max().item() <= 0, f"seq {b} {name}: varlen autograd beyond (B2)"
            assert ((f - r).abs() - bound).max().item() <= 0, f"seq {b} {name}: flash_attn_func beyond (B2)"
            assert ((a - f).abs() - 2 * bound).max().item() <= 0, f"seq {b} {name}"


# ---- 6. graph capture --------------------------------------------------------------------------------------------------------

def test_graph_capture_reads_lengths_on_device(tfa, dev):
    from tiny_flash_attention_amd import ops

    dtype, H, Hk, D, causal = torch.bfloat16, 4, 2, 128, True
    max_q, max_k, B = 512, 512, 4
    tq, tk = B * max_q, B * max_k
    q = rnd((tq, H, D), dtype, 51).to(dev)
    k = rnd((tk, Hk, D), dtype, 52).to(dev)
    v = rnd((tk, Hk, D), dtype, 53).to(dev)
    do = rnd((tq, H, D), dtype, 54).to(dev)
    cq_s = cu_of([512, 100, 300, 7]).to(dev)             # static device buffers the graph reads
    ck_s = cu_of([512, 400, 1, 200]).to(dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                           # warm-up outside the capture (first-use work of the runtime)
        ops.flash_attn_varlen_fwd(q, k, v, cq_s, ck_s, max_q, max_k, causal)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, lse = ops.flash_attn_varlen_fwd(q, k, v, cq_s, ck_s, max_q, max_k, causal)
        dq, dk, dv = ops.flash_attn_varlen_bwd(q, k, v, out, lse, do, cq_s, ck_s, max_q, max_k, causal)
    new_q, new_k = cu_of([33, 512, 129, 400]), cu_of([512, 64, 300, 256])   # different lengths, the same maxima
    cq_s.copy_(new_q.to(dev))
    ck_s.copy_(new_k.to(dev))
    g.replay()
    torch.cuda.synchronize()
    cq_e, ck_e = new_q.to(dev), new_k.to(dev)
    out_e, lse_e = ops.flash_attn_varlen_fwd(q, k, v, cq_e, ck_e, max_q, max_k, causal)
    ge = ops.flash_attn_varlen_bwd(q, k, v, out_e, lse_e, do, cq_e, ck_e, max_q, max_k, causal)
    torch.cuda.synchronize()
    nq, nk = int(new_q[-1]), int(new_k[-1])
    assert torch.equal(out[:nq], out_e[:nq]) and torch.equal(lse[:, :nq], lse_e[:, :nq])
    assert torch.equal(dq, ge[0]) and torch.equal(dk[:nk], ge[1][:nk]) and torch.equal(dv[:nk], ge[2][:nk])
