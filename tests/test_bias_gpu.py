"""GPU tests of the dense additive bias / mask (include/tfa.h: tfa_fwd_bias, tfa_bwd_bias; ops attn_bias=).

The reference is written in this file: fp64 scores scale * q.k + bias[b,h,i,j] (the bias as stored, broadcast over batch / heads), FlashAttention-2's
window / causal mask, logsumexp (INCLUDING the bias), P @ v and A = P @ |v|; rows without a finite score -> out 0, lse +inf; gradients by fp64 autograd
of the same expression.  Inputs normal(0, 0.5), the bias normal(0, 1) in its own dtype, all seeded.
Bars (include/tfa.h, "which tolerance each path guarantees", as the ALiBi tests state them): 16-bit out |d| <= 1e-2; fp32 out |d| <= eps16 * A + 1e-6;
LSE +inf exactly on empty rows, elsewhere |d| <= 1e-4 * max(1, |ref|); gradients max|d| <= 1e-2 * max(1, max|ref|) (16 bit) and
<= 8 * eps16 * max(1, max|ref|) (fp32), finite, bit-equal across two runs.
  1. forward vs fp64 (a 256-row block boundary, a partial last tile, the wrapper's padding path, rows without keys; variants, dtypes, head dims, GQA,
     the four broadcast shapes, q's dtype and fp32, causal, a window);  2. -inf masks placed by construction, and a bool mask through flash_attn_func;
  3. a re-base: +30 on the last tile's keys at Nk = 2048;  4. backward vs fp64 autograd;  5. attn_bias=None: today's bits;  6. one graph capture, the
     bias overwritten in place.
"""
import math

import pytest
import torch

import form_ref

pytestmark = pytest.mark.gpu

B, H, HK = 2, 4, 2
SHAPES = [(320, 320), (70, 203), (257, 64)]
NEG = -math.inf


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from tiny_flash_attention_amd import _lib

    _lib.lib()
    return _lib


def rnd(shape, dtype, seed, std=0.5):
    g = torch.Generator().manual_seed(seed)
    return torch.empty(shape, dtype=torch.float32).normal_(0.0, std, generator=g).to(dtype)


def window_mask(Nq, Nk, left, right):
    i = torch.arange(Nq).view(-1, 1)
    j = torch.arange(Nk).view(1, -1)
    shift = Nk - Nq
    m = torch.ones(Nq, Nk, dtype=torch.bool)
    if left >= 0:
        m &= j >= i + shift - left
    if right >= 0:
        m &= j <= i + shift + right
    return m


def scores64(q64, k64, bias, left, right, sc):
    Nq, Nk = q64.shape[2], k64.shape[2]
    s = (q64 @ k64.transpose(-1, -2)) * sc + bias.detach().double().cpu()
    return s.masked_fill(~window_mask(Nq, Nk, left, right), NEG)


def ref64(q, k, v, bias, left, right, sc):
    """q (B,H,Nq,D), k / v (B,Hk,Nk,D), bias broadcastable to (B,H,Nq,Nk) -> out64, lse64, A (sum_j P |v|), on the CPU in fp64."""
    q, k, v = q.double().cpu(), k.double().cpu(), v.double().cpu()
    G = q.shape[1] // k.shape[1]
    k, v = k.repeat_interleave(G, dim=1), v.repeat_interleave(G, dim=1)
    s = scores64(q, k, bias, left, right, sc)
    lse = torch.logsumexp(s, dim=-1)
    p = torch.nan_to_num(torch.exp(s - lse.unsqueeze(-1)), nan=0.0)
    lse = lse.masked_fill(torch.isneginf(lse), math.inf)
    return p @ v, lse, p @ v.abs()


def ref_grads(q, k, v, dout, bias, left, right, sc):
    q64, k64, v64 = (t.double().cpu().requires_grad_(True) for t in (q, k, v))
    G = q.shape[1] // k.shape[1]
    kk, vv = k64.repeat_interleave(G, dim=1), v64.repeat_interleave(G, dim=1)
    s = scores64(q64, kk, bias, left, right, sc)
    empty = torch.isneginf(s).all(dim=-1, keepdim=True)   # (a row of -inf alone: softmax's backward would give NaN — such a row is P = 0 by definition)
    p = torch.softmax(torch.where(empty, torch.zeros_like(s), s), dim=-1) * (~empty)
    (p @ vv).backward(dout.double().cpu())
    return q64.grad, k64.grad, v64.grad


def check_fwd(out, lse, ref, dtype, f32, out16=True):
    r, lref, A = ref
    o = out.double().cpu()
    assert not bool(torch.isnan(o).any()) and not bool(torch.isnan(lse).any()), "NaN in the result"
    if f32:
        eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
        ex = ((o - r).abs() - (eps * A + 1e-6)).max().item()
        print(f"fp32 out: max(|d| - (eps16 * A + 1e-6)) = {ex:.3e}")
        assert ex <= 0, f"fp32 out exceeds eps16 * A + 1e-6 by {ex:.3e}"
    elif out16:
        err = (o - r).abs().max().item()
        print(f"16-bit out: max|d| = {err:.3e}")
        assert err <= 1e-2, f"out: max|d| = {err:.3e}"
    l = lse.double().cpu()
    inf = torch.isinf(lref)
    assert torch.equal(torch.isinf(l), inf) and bool((l[inf] > 0).all()), "lse must be +inf exactly on rows without a finite score"
    if (~inf).any():
        e = ((l[~inf] - lref[~inf]).abs() / lref[~inf].abs().clamp_min(1.0)).max().item()
        print(f"lse: max|d| / max(1, |ref|) = {e:.3e}")
        assert e <= 1e-4, f"lse: max|d| / max(1, |ref|) = {e:.3e}"
    assert bool((o[inf.unsqueeze(-1).expand_as(o)] == 0).all()), "rows without a finite score must be exactly 0"


def check_bwd(g32, g16, ref, dtype, bounds=None):
    eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    if bounds is not None:  # element by element: (B1) / (B2) with form_ref.bwd_bounds
        form_ref.check_grads(g32, g16, ref, bounds, dtype, "bias")
    for name, a32, a16, r in zip(("dq", "dk", "dv"), g32, g16, ref):
        a32c, a16c = a32.double().cpu(), a16.double().cpu()
        assert bool(torch.isfinite(a16c).all()) and bool(torch.isfinite(a32c).all()), name
        scale = max(1.0, r.abs().max().item())
        e16, e32 = (a16c - r).abs().max().item(), (a32c - r).abs().max().item()
        print(f"{name}: 16-bit max|d| = {e16:.3e}, fp32 max|d| = {e32:.3e}, max|ref| = {r.abs().max().item():.3e}")
        assert e16 <= 1e-2 * scale, f"{name}: {e16:.3e}"
        assert e32 <= 8 * eps * scale, f"{name} fp32: {e32:.3e}"


def forced(lib, variant):
    class _F:
        def __enter__(self):
            lib.set_variant(variant)

        def __exit__(self, *a):
            lib.set_variant(-1)
    return _F()


def eff_window(causal, window):
    return (window[0], 0) if causal else window


def qkv(Nq, Nk, D, dtype, seed):
    return rnd((B, H, Nq, D), dtype, seed), rnd((B, HK, Nk, D), dtype, seed + 1), rnd((B, HK, Nk, D), dtype, seed + 2)


def fwd(q, k, v, causal, sc, bias, window=(-1, -1), out_f32=False):
    from tiny_flash_attention_amd import ops

    o, l = ops.flash_attn_fwd(q, k, v, causal, sc, out_f32=out_f32, window_size=window, attn_bias=bias)
    torch.cuda.synchronize()
    return o, l


def masked_bias(Nq, Nk, shape, dtype, seed):
    """normal(0, 1) with -inf placed by construction: rows 3, 64, 255, 256 fully masked; keys 0..63 masked for every row of the first 256-row block (its first
    visited tile is empty); rows 32..63 x keys 64..127 (a whole wave's tile); the last tile; key 5 for every row (an unseen key); a seeded random half of the rest."""
    bias = rnd((shape[0], shape[1], Nq, Nk), torch.float32, seed, std=1.0)
    g = torch.Generator().manual_seed(seed + 100)
    m = torch.rand((shape[0], shape[1], Nq, Nk), generator=g) < 0.5
    for r in (3, 64, 255, 256):
        if r < Nq:
            m[:, :, r, :] = True
    m[:, :, :256, :64] = True
    if Nk >= 128:
        m[:, :, 32:64, 64:128] = True
    if Nk > 64:
        m[:, :, :, (Nk - 1) // 64 * 64:] = True
    else:
        m[:, :, 256:, 1::2] = False                      # (one tile only: the rows behind the first block keep some keys)
    m[:, :, :, 5] = True
    return bias.masked_fill(m, NEG).to(dtype)


# ---- 1. forward against fp64 ------------------------------------------------------------------------------------------------------------
# (Nq, Nk) x variant x mask, the other axes rotated through them so that every value of every axis meets every shape: dtype, head dim, the four broadcast
# shapes, the bias dtype (q's / fp32)
MASKS = [(False, (-1, -1)), (True, (-1, -1)), (False, (48, 0))]
DTYPES = [torch.bfloat16, torch.float16]
DIMS = [64, 128, 40]
BSHAPES = [(B, H), (1, H), (B, 1), (1, 1)]
FWD_CASES = []
for si, (nq_, nk_) in enumerate(SHAPES):
    for vi, variant_ in enumerate((30, 32)):
        for mi, (causal_, window_) in enumerate(MASKS):
            for rep in range(2):
                n = len(FWD_CASES)
                FWD_CASES.append((nq_, nk_, variant_, causal_, window_, DTYPES[(n + si) % 2], DIMS[(n + vi) % 3], BSHAPES[(n + mi + rep) % 4], (n // 2 + rep) % 2 == 0))


@pytest.mark.parametrize("Nq,Nk,variant,causal,window,dtype,D,bshape,bias_f32", FWD_CASES)
def test_fwd_vs_fp64(lib, dev, Nq, Nk, variant, causal, window, dtype, D, bshape, bias_f32):
    q, k, v = qkv(Nq, Nk, D, dtype, 11)
    sc = 1.0 / math.sqrt(D)
    bias = rnd((bshape[0], bshape[1], Nq, Nk), torch.float32 if bias_f32 else dtype, 14, std=1.0)
    w = eff_window(causal, window)
    ref = ref64(q, k, v, bias, w[0], w[1], sc)
    qd, kd, vd, bd = q.to(dev), k.to(dev), v.to(dev), bias.to(dev)
    with forced(lib, variant):
        o, l = fwd(qd, kd, vd, causal, sc, bd, window)
        o32, l32 = fwd(qd, kd, vd, causal, sc, bd, window, out_f32=True)
    check_fwd(o, l, ref, dtype, False)
    check_fwd(o32, l32, ref, dtype, True)


# ---- 2. masks: -inf from memory ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("variant", [30, 32])
@pytest.mark.parametrize("Nq,Nk", SHAPES)
@pytest.mark.parametrize("dtype,D,bshape,bias_f32", [(torch.bfloat16, 128, (B, H), False), (torch.float16, 64, (1, H), True)])
def test_masks_vs_fp64(lib, dev, causal, variant, Nq, Nk, dtype, D, bshape, bias_f32):
    q, k, v = qkv(Nq, Nk, D, dtype, 21)
    sc = 1.0 / math.sqrt(D)
    bias = masked_bias(Nq, Nk, bshape, torch.float32 if bias_f32 else dtype, 24)
    w = eff_window(causal, (-1, -1))
    ref = ref64(q, k, v, bias, w[0], w[1], sc)
    assert bool(torch.isinf(ref[1]).any()), "the case must hold rows without a finite score"
    qd, kd, vd, bd = q.to(dev), k.to(dev), v.to(dev), bias.to(dev)
    with forced(lib, variant):
        o, l = fwd(qd, kd, vd, causal, sc, bd)
        o32, l32 = fwd(qd, kd, vd, causal, sc, bd, out_f32=True)
    check_fwd(o, l, ref, dtype, False)
    check_fwd(o32, l32, ref, dtype, True)


@pytest.mark.parametrize("Nq,Nk", SHAPES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_bool_mask_through_flash_attn_func(lib, dev, Nq, Nk, dtype):
    import tiny_flash_attention_amd as tfa

    D = 64
    q, k, v = qkv(Nq, Nk, D, dtype, 31)
    keep = torch.isfinite(masked_bias(Nq, Nk, (B, 1), torch.float32, 34))           # True = attend
    zero_inf = torch.zeros(keep.shape).masked_fill(~keep, NEG)
    ref = ref64(q, k, v, zero_inf, -1, -1, 1.0 / math.sqrt(D))
    out = tfa.flash_attn_func(q.transpose(1, 2).to(dev), k.transpose(1, 2).to(dev), v.transpose(1, 2).to(dev), attn_bias=keep.to(dev))
    torch.cuda.synchronize()
    o = out.transpose(1, 2).double().cpu()
    assert not bool(torch.isnan(o).any())
    err = (o - ref[0]).abs().max().item()
    print(f"16-bit out: max|d| = {err:.3e}")
    assert err <= 1e-2
    empty = torch.isinf(ref[1])
    assert bool(empty.any()) and bool((o[empty.unsqueeze(-1).expand_as(o)] == 0).all())


# ---- 3. re-base: the last tile carries +30 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [30, 32])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_rebase_on_the_last_tile(lib, dev, variant, dtype):
    """Every row's reference is set by 31 tiles of ordinary scores; the last tile's keys then lie 30 above them (43 in the log2 domain): the lazy rule re-bases
    there.  The rows become peaked: the fp32-out bound and the LSE only, as the steep-slope ALiBi cases."""
    Nq, Nk, D = 64, 2048, 128
    q, k, v = qkv(Nq, Nk, D, dtype, 41)
    sc = 1.0 / math.sqrt(D)
    bias = torch.zeros(1, 1, Nq, Nk, dtype=dtype)
    bias[..., Nk - 64:] = 30.0
    ref = ref64(q, k, v, bias, -1, -1, sc)
    with forced(lib, variant):
        o32, l32 = fwd(q.to(dev), k.to(dev), v.to(dev), False, sc, bias.to(dev), out_f32=True)
    check_fwd(o32, l32, ref, dtype, True)


# ---- 4. backward against fp64 autograd --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("Nq,Nk", [(192, 192), (70, 203)])
@pytest.mark.parametrize("dtype,D,bshape,bias_f32", [(torch.bfloat16, 128, (B, H), False), (torch.float16, 64, (1, H), True),
                                                     (torch.bfloat16, 64, (1, 1), True), (torch.float16, 128, (B, 1), False)])
def test_bwd_vs_fp64(lib, dev, causal, Nq, Nk, dtype, D, bshape, bias_f32):
    from tiny_flash_attention_amd import ops
    import tiny_flash_attention_amd as tfa

    q, k, v = qkv(Nq, Nk, D, dtype, 51)
    dout = rnd((B, H, Nq, D), dtype, 54)
    sc = 1.0 / math.sqrt(D)
    bias = masked_bias(Nq, Nk, bshape, torch.float32 if bias_f32 else dtype, 55)
    w = eff_window(causal, (-1, -1))
    ref = ref_grads(q, k, v, dout, bias, w[0], w[1], sc)
    qd, kd, vd, dd, bd = q.to(dev), k.to(dev), v.to(dev), dout.to(dev), bias.to(dev)
    o, l = fwd(qd, kd, vd, causal, sc, bd)
    g16 = ops.flash_attn_bwd(qd, kd, vd, o, l, dd, causal, sc, attn_bias=bd)
    g32 = ops.flash_attn_bwd(qd, kd, vd, o, l, dd, causal, sc, grad_f32=True, attn_bias=bd)
    again = ops.flash_attn_bwd(qd, kd, vd, o, l, dd, causal, sc, attn_bias=bd)
    torch.cuda.synchronize()
    check_bwd(g32, g16, ref, dtype, bounds=form_ref.bwd_bounds(q, k, v, o, dout, sc, bias=bias, window=w))
    for a, b in zip(g16, again):
        assert torch.equal(a, b), "the backward must be deterministic"
    # fully masked rows get no dq, keys nobody sees get no dk / dv: exactly 0
    empty = torch.isinf(ref64(q, k, v, bias, w[0], w[1], sc)[1])                    # (B, H, Nq)
    assert bool(empty.any())
    for g in (g16[0], g32[0]):
        assert bool((g.cpu()[empty.unsqueeze(-1).expand_as(g)] == 0).all()), "dq of fully masked rows"
    for g in (g16[1], g32[1], g16[2], g32[2]):
        assert bool((g.cpu()[:, :, 5, :] == 0).all()), "dk / dv of a key every row masks"
        if Nk > 64:
            assert bool((g.cpu()[:, :, (Nk - 1) // 64 * 64:, :] == 0).all()), "dk / dv of the masked last tile"
    # ... and through autograd: flash_attn_func(...).backward
    qa, ka, va = (t.transpose(1, 2).detach().clone().requires_grad_(True) for t in (qd, kd, vd))
    out = tfa.flash_attn_func(qa, ka, va, causal=causal, attn_bias=bd)
    out.backward(dd.transpose(1, 2))
    torch.cuda.synchronize()
    for a, b in zip(g16, (qa.grad, ka.grad, va.grad)):
        assert torch.equal(a, b.transpose(1, 2)), "flash_attn_func's backward is ops.flash_attn_bwd on the same tensors"


# ---- 5. attn_bias=None is today's call, bit for bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [(-1, -1), (100, 0)])
@pytest.mark.parametrize("causal", [False, True])
def test_none_is_todays_call(lib, dev, window, causal):
    from tiny_flash_attention_amd import ops
    import tiny_flash_attention_amd as tfa

    dtype, Nq, Nk, D = torch.bfloat16, 300, 700, 64
    q, k, v = (t.to(dev) for t in qkv(Nq, Nk, D, dtype, 61))
    dout = rnd((B, H, Nq, D), dtype, 64).to(dev)
    sc = 1.0 / math.sqrt(D)
    o0, l0 = ops.flash_attn_fwd(q, k, v, causal, sc, window_size=window)
    o1, l1 = ops.flash_attn_fwd(q, k, v, causal, sc, window_size=window, attn_bias=None)
    assert torch.equal(o0, o1) and torch.equal(l0, l1)
    g0 = ops.flash_attn_bwd(q, k, v, o0, l0, dout, causal, sc, window_size=window)
    g1 = ops.flash_attn_bwd(q, k, v, o0, l0, dout, causal, sc, window_size=window, attn_bias=None)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    grads = []
    for kw in ({}, {"attn_bias": None}):
        qa, ka, va = (t.transpose(1, 2).detach().clone().requires_grad_(True) for t in (q, k, v))
        out = tfa.flash_attn_func(qa, ka, va, causal=causal, window_size=window, **kw)
        out.backward(dout.transpose(1, 2))
        grads.append((out.detach(), qa.grad, ka.grad, va.grad))
    for a, b in zip(*grads):
        assert torch.equal(a, b)


# ---- 6. one graph capture; the bias overwritten in place -----------------------------------------------------------------------------------
def test_graph_replay_reads_the_new_bias(lib, dev):
    """The bias is read by the kernels only: a captured forward replayed after the tensor was overwritten in place computes with the new values.  One
    straight line on one stream."""
    from tiny_flash_attention_amd import ops

    dtype, Nq, Nk, D = torch.bfloat16, 320, 320, 128
    q, k, v = (t.to(dev) for t in qkv(Nq, Nk, D, dtype, 71))
    sc = 1.0 / math.sqrt(D)
    bias = rnd((1, H, Nq, Nk), dtype, 74, std=1.0).to(dev)
    new = masked_bias(Nq, Nk, (1, H), dtype, 75).to(dev)
    out = torch.empty_like(q)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.flash_attn_fwd(q, k, v, True, sc, out=out, attn_bias=bias)              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, lse = ops.flash_attn_fwd(q, k, v, True, sc, out=out, attn_bias=bias)
    bias.copy_(new)
    graph.replay()
    torch.cuda.synchronize()
    o_ref, l_ref = ops.flash_attn_fwd(q, k, v, True, sc, attn_bias=new)
    torch.cuda.synchronize()
    assert torch.equal(out, o_ref) and torch.equal(lse, l_ref)
    check_fwd(out, lse, ref64(q, k, v, new, -1, 0, sc), dtype, False)
