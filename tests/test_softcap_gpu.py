"""GPU tests of soft-capping (include/tfa.h: tfa_fwd_softcap, tfa_bwd_softcap and the varlen forms; ops softcap=).

The reference is written in this file: fp64 scores S = c * tanh(scale * q.k / c) - slope[b,h] * |i + shift - j| (shift = Nk - Nq; the cap first, then the
bias), FlashAttention-2's window / causal mask, logsumexp of S, P @ v and A = P @ |v|; rows that see nothing -> out 0, lse +inf; gradients by fp64 autograd
of the same expression (so the chain rule through tanh is the reference's, not restated).
Bars (include/tfa.h, "which tolerance each path guarantees"): 16-bit out |d| <= 1e-2; fp32 out |d| <= eps16 * A + 1e-6; LSE +inf exactly on rows that see
no key, elsewhere |d| <= 1e-4 * max(1, |ref|); gradients max|d| <= 1e-2 * max(1, max|ref|) (16 bit) and <= 8 * eps16 * max(1, max|ref|) (fp32), finite,
bit-equal over two runs.

A cap nobody applied must fail: every *bite* case first asserts, on the CPU and in fp64, that the reference computed WITHOUT the cap misses each bar the
case asserts by at least 10x on the case's own inputs (bite_fwd / bite_bwd) — a condition on the inputs, not on the kernels.  One backward case asserts
the same for a straight-through reference (capped forward, identity backward through the cap), so the tests demonstrably cover the 1 - tanh^2 factor.
  1. softcap=0.0: the bits of today's calls;  2. forward vs fp64, bite;  3. near-linear and mid regime (softcap 30 / 50 / 20);  4. saturation (std 8);
  5. with alibi_slopes, windows, both; zero slopes = no slopes in bits;  6. backward vs fp64 autograd, bite, derivative-omitted check;
  7. flash_attn_func and flash_attn_varlen_func;  8. one CUDA-graph capture of forward + backward.
"""
import math

import pytest
import torch

import form_ref

pytestmark = pytest.mark.gpu


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


def std_slopes(H, mult=1.0):
    return torch.tensor([mult * 2.0 ** (-8.0 * (h + 1) / H) for h in range(H)], dtype=torch.float32)


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


def bias64(slopes, B, H, Nq, Nk):
    """-slope[b,h] * |i + shift - j| as (B,H,Nq,Nk) fp64; slopes None / (H,) / (B,H)."""
    if slopes is None:
        return torch.zeros(1, 1, Nq, Nk, dtype=torch.float64)
    s = slopes.detach().double().cpu()
    s = s.view(1, H, 1, 1) if s.dim() == 1 else s.view(B, H, 1, 1)
    i = torch.arange(Nq, dtype=torch.float64).view(-1, 1)
    j = torch.arange(Nk, dtype=torch.float64).view(1, -1)
    return -s * (i + (Nk - Nq) - j).abs()


def scores64(q64, k64, cap, slopes, left, right, sc, straight_through=False):
    """S: the cap on the scaled scores (cap = 0: none), then the bias, then the mask.  straight_through: the capped values with the identity's gradient."""
    B, H, Nq, _ = q64.shape
    Nk = k64.shape[2]
    x = (q64 @ k64.transpose(-1, -2)) * sc
    if cap:
        capped = cap * torch.tanh(x / cap)
        x = x + (capped - x).detach() if straight_through else capped
    s = x + bias64(slopes, B, H, Nq, Nk)
    m = window_mask(Nq, Nk, left, right)
    return s.masked_fill(~m, -math.inf), m


def ref64(q, k, v, cap, slopes, left, right, sc):
    """q (B,H,Nq,D), k / v (B,Hk,Nk,D) -> out64, lse64, A (sum_j P |v|), on the CPU in fp64."""
    q, k, v = q.double().cpu(), k.double().cpu(), v.double().cpu()
    G = q.shape[1] // k.shape[1]
    k, v = k.repeat_interleave(G, dim=1), v.repeat_interleave(G, dim=1)
    s, m = scores64(q, k, cap, slopes, left, right, sc)
    lse = torch.logsumexp(s, dim=-1)
    p = torch.nan_to_num(torch.exp(s - lse.unsqueeze(-1)), nan=0.0)
    empty = ~m.any(dim=-1)
    lse = lse.masked_fill(empty.view(1, 1, -1).expand_as(lse), math.inf)
    return p @ v, lse, p @ v.abs()


def ref_grads(q, k, v, dout, cap, slopes, left, right, sc, straight_through=False):
    q64, k64, v64 = (t.double().cpu().requires_grad_(True) for t in (q, k, v))
    G = q.shape[1] // k.shape[1]
    kk, vv = k64.repeat_interleave(G, dim=1), v64.repeat_interleave(G, dim=1)
    s, _ = scores64(q64, kk, cap, slopes, left, right, sc, straight_through)
    p = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)
    (p @ vv).backward(dout.double().cpu())
    return q64.grad, k64.grad, v64.grad


def eps16(dtype):
    return 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11


def bite_fwd(q, k, v, cap, slopes, left, right, sc, dtype, ref=None):
    """The inputs' condition of a forward bite case: the fp64 reference WITHOUT the cap misses the 16-bit bar (1e-2), the fp32 bar (eps16 * A + 1e-6,
    somewhere) and the LSE bar (1e-4 * max(1, |ref|)) by at least 10x each."""
    ref, lref, A = ref if ref is not None else ref64(q, k, v, cap, slopes, left, right, sc)
    un, lun, _ = ref64(q, k, v, 0.0, slopes, left, right, sc)
    d = (un - ref).abs()
    fin = ~torch.isinf(lref)
    dl = ((lun[fin] - lref[fin]).abs() / lref[fin].abs().clamp_min(1.0)).max().item()
    r32 = (d / (eps16(dtype) * A + 1e-6)).max().item()
    print(f"bite (no cap applied): out max|d| = {d.max().item():.3f} ({d.max().item() / 1e-2:.0f}x the 16-bit bar), {r32:.0f}x the fp32 bar, lse {dl / 1e-4:.0f}x")
    assert d.max().item() >= 10 * 1e-2, f"not a bite case: uncapped reference within {d.max().item():.3e} of the capped one"
    assert r32 >= 10, f"not a bite case for the fp32 bar: {r32:.1f}x"
    assert dl >= 10 * 1e-4, f"not a bite case for the LSE bar: {dl:.3e}"


def bite_bwd(ref, other, dtype, what):
    """The inputs' condition of a backward bite case: `other` (fp64 gradients of a reference that lacks the cap, or its derivative) misses the 16-bit bar
    (1e-2 * max(1, max|ref|)) and the fp32 bar (8 * eps16 * max(1, max|ref|)) by at least 10x — for dq and dk always, for dv where `other` changes it."""
    for name, r, u in zip(("dq", "dk", "dv"), ref, other):
        scale = max(1.0, r.abs().max().item())
        d = (u - r).abs().max().item()
        print(f"bite ({what}): {name} max|d| / max(1, max|ref|) = {d / scale:.3f} ({d / scale / 1e-2:.0f}x the 16-bit bar, {d / scale / (8 * eps16(dtype)):.0f}x the fp32 bar)")
        if name == "dv" and what == "derivative omitted":
            continue                                            # (dv does not pass through the cap's derivative)
        assert d >= 10 * 1e-2 * scale, f"not a bite case ({what}): {name} {d / scale:.3e}"
        assert d >= 10 * 8 * eps16(dtype) * scale, f"not a bite case for the fp32 bar ({what}): {name} {d / scale:.3e}"


def check_fwd(out, lse, q, k, v, cap, slopes, left, right, sc, dtype, f32, out16=True, ref=None):
    ref, lref, A = ref if ref is not None else ref64(q, k, v, cap, slopes, left, right, sc)
    o = out.double().cpu()
    assert bool(torch.isfinite(o).all()), "out must be finite"
    if f32:
        ex = ((o - ref).abs() - (eps16(dtype) * A + 1e-6)).max().item()
        print(f"fp32 out: max(|d| - (eps16 * A + 1e-6)) = {ex:.3e}")
        assert ex <= 0, f"fp32 out exceeds eps16 * A + 1e-6 by {ex:.3e}"
    elif out16:
        err = (o - ref).abs().max().item()
        print(f"16-bit out: max|d| = {err:.3e}")
        assert err <= 1e-2, f"out: max|d| = {err:.3e}"
    l = lse.double().cpu()
    assert not bool(torch.isnan(l).any()), "lse must not be NaN"
    inf = torch.isinf(lref)
    assert torch.equal(torch.isinf(l), inf) and bool((l[inf] > 0).all()), "lse must be +inf exactly on rows that see no key"
    if (~inf).any():
        e = ((l[~inf] - lref[~inf]).abs() / lref[~inf].abs().clamp_min(1.0)).max().item()
        print(f"lse: max|d| / max(1, |ref|) = {e:.3e} (max|ref| = {lref[~inf].abs().max().item():.1f})")
        assert e <= 1e-4, f"lse: max|d| / max(1, |ref|) = {e:.3e}"
    assert bool((o[inf.unsqueeze(-1).expand_as(o)] == 0).all()), "rows that see no key must be 0"


def check_bwd(g32, g16, ref, dtype, bounds=None):
    if bounds is not None:  # element by element: (B1) / (B2) with form_ref.bwd_bounds
        form_ref.check_grads(g32, g16, ref, bounds, dtype, "softcap")
    for name, a32, a16, r in zip(("dq", "dk", "dv"), g32, g16, ref):
        a32c, a16c = a32.double().cpu(), a16.double().cpu()
        assert bool(torch.isfinite(a16c).all()) and bool(torch.isfinite(a32c).all()), name
        mref = r.abs().max().item()
        scale = max(1.0, mref)
        e16, e32 = (a16c - r).abs().max().item(), (a32c - r).abs().max().item()
        print(f"{name}: 16-bit max|d| = {e16:.3e}, fp32 max|d| = {e32:.3e}, max|ref| = {mref:.3e}, max|d| / max|ref| = {e16 / mref:.3e} (16 bit) {e32 / mref:.3e} (fp32)")
        assert e16 <= 1e-2 * scale, f"{name}: {e16:.3e}"
        assert e32 <= 8 * eps16(dtype) * scale, f"{name} fp32: {e32:.3e}"


def fwd(q, k, v, causal, sc, cap, slopes=None, window=(-1, -1), out_f32=False):
    from tiny_flash_attention_amd import ops

    o, l = ops.flash_attn_fwd(q, k, v, causal, sc, out_f32=out_f32, window_size=window, alibi_slopes=slopes, softcap=cap)
    torch.cuda.synchronize()
    return o, l


def forced(lib, variant):
    class _F:
        def __enter__(self):
            lib.set_variant(variant)

        def __exit__(self, *a):
            lib.set_variant(-1)
    return _F()


def cu_of(lens):
    c = [0]
    for n in lens:
        c.append(c[-1] + n)
    return torch.tensor(c, dtype=torch.int32)


def eff_window(causal, window):
    return (window[0], 0) if causal else window


def qkv(B, H, Hk, Nq, Nk, D, dtype, seed, std, dev):
    """q, k at `std`, v at 0.5 (16-bit rounded: the kernels and the reference see the same values)."""
    return (rnd((B, H, Nq, D), dtype, seed, std).to(dev), rnd((B, Hk, Nk, D), dtype, seed + 1, std).to(dev), rnd((B, Hk, Nk, D), dtype, seed + 2, 0.5).to(dev))


# ---- 1. softcap=0.0 is today's call, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_slopes", [False, True])
@pytest.mark.parametrize("window", [(-1, -1), (100, 0)])
@pytest.mark.parametrize("causal", [False, True])
def test_zero_is_todays_call_fixed(lib, dev, window, causal, with_slopes):
    from tiny_flash_attention_amd import ops

    dtype, B, H, Nq, Nk, D = torch.bfloat16, 2, 4, 300, 700, 64
    q, k, v = (rnd((B, H, n, D), dtype, s).to(dev) for s, n in ((1, Nq), (2, Nk), (3, Nk)))
    dout = rnd((B, H, Nq, D), dtype, 4).to(dev)
    sc = 1.0 / math.sqrt(D)
    kw = dict(window_size=window)
    if with_slopes:
        kw["alibi_slopes"] = std_slopes(H).to(dev)
    o0, l0 = ops.flash_attn_fwd(q, k, v, causal, sc, **kw)
    o1, l1 = ops.flash_attn_fwd(q, k, v, causal, sc, softcap=0.0, **kw)
    assert torch.equal(o0, o1) and torch.equal(l0, l1)
    g0 = ops.flash_attn_bwd(q, k, v, o0, l0, dout, causal, sc, **kw)
    g1 = ops.flash_attn_bwd(q, k, v, o0, l0, dout, causal, sc, softcap=0.0, **kw)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)


@pytest.mark.parametrize("with_slopes", [False, True])
@pytest.mark.parametrize("window", [(-1, -1), (64, 0)])
def test_zero_is_todays_call_varlen(lib, dev, window, with_slopes):
    from tiny_flash_attention_amd import ops

    dtype, H, D = torch.bfloat16, 4, 64
    lq, lk = [100, 200, 37], [150, 200, 90]
    cq, ck = cu_of(lq).to(dev), cu_of(lk).to(dev)
    q, k, v = rnd((sum(lq), H, D), dtype, 5).to(dev), rnd((sum(lk), H, D), dtype, 6).to(dev), rnd((sum(lk), H, D), dtype, 7).to(dev)
    dout = rnd((sum(lq), H, D), dtype, 8).to(dev)
    kw = dict(window_size=window)
    if with_slopes:
        kw["alibi_slopes"] = std_slopes(H).to(dev)
    o0, l0 = ops.flash_attn_varlen_fwd(q, k, v, cq, ck, 200, 200, True, None, **kw)
    o1, l1 = ops.flash_attn_varlen_fwd(q, k, v, cq, ck, 200, 200, True, None, softcap=0.0, **kw)
    assert torch.equal(o0, o1) and torch.equal(l0, l1)
    g0 = ops.flash_attn_varlen_bwd(q, k, v, o0, l0, dout, cq, ck, 200, 200, True, None, **kw)
    g1 = ops.flash_attn_varlen_bwd(q, k, v, o0, l0, dout, cq, ck, 200, 200, True, None, softcap=0.0, **kw)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)


# ---- 2. forward against fp64, bite ---------------------------------------------------------------------------------------------------------
# (std of q and k, softcap): the pairs for which the uncapped reference is at least 10x the 16-bit bar away; each is used with both dtypes
PAIRS = [(1.0, 1.0), (1.0, 5.0), (2.0, 5.0)]
FWD_BITE = [
    # D, Nq, Nk, causal, window, variant, pair
    (64, 300, 700, True, (-1, -1), -1, 1),
    (128, 300, 700, True, (-1, -1), -1, 1),
    (128, 300, 700, True, (-1, -1), -1, 0),
    (64, 300, 700, True, (-1, -1), -1, 2),
    (40, 517, 517, False, (-1, -1), -1, 1),
    (96, 517, 517, True, (-1, -1), -1, 0),
    (96, 700, 700, False, (-1, -1), 30, 2),
    (128, 700, 700, True, (-1, -1), 30, 1),
    (128, 700, 700, False, (-1, -1), 32, 1),
    (64, 700, 700, True, (-1, -1), 32, 0),
    (128, 900, 333, True, (-1, -1), -1, 1),            # Nq > Nk: the first Nq - Nk rows see nothing
    (64, 900, 333, False, (100, 50), 30, 2),
    (128, 300, 900, False, (200, 77), -1, 2),          # windows with both edges
    (40, 700, 700, False, (128, 128), 32, 2),
    (96, 700, 700, True, (300, 0), -1, 2),
    (64, 300, 900, False, (-1, 64), -1, 2),            # (std 1 reaches 9.96x here: std 2)
    (128, 700, 700, False, (64, -1), -1, 1),
]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D,Nq,Nk,causal,window,variant,pair", FWD_BITE)
def test_fwd_vs_fp64_bite(lib, dev, dtype, D, Nq, Nk, causal, window, variant, pair):
    std, cap = PAIRS[pair]
    B, H, Hk = 1, 4, 2                                                                       # GQA
    q, k, v = qkv(B, H, Hk, Nq, Nk, D, dtype, 100 + D, std, dev)
    sc = 1.0 / math.sqrt(D)
    w = eff_window(causal, window)
    ref = ref64(q, k, v, cap, None, w[0], w[1], sc)
    bite_fwd(q, k, v, cap, None, w[0], w[1], sc, dtype, ref)
    with forced(lib, variant):
        o, l = fwd(q, k, v, causal, sc, cap, None, window)
        o32, l32 = fwd(q, k, v, causal, sc, cap, None, window, out_f32=True)
    check_fwd(o, l, q, k, v, cap, None, w[0], w[1], sc, dtype, False, ref=ref)
    check_fwd(o32, l32, q, k, v, cap, None, w[0], w[1], sc, dtype, True, ref=ref)


# ---- 3. near-linear and mid regime: the values models use; guards the cancellation in 1 - 2r for small arguments ------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("std,cap", [(0.5, 30.0), (0.5, 50.0), (1.0, 20.0)])
@pytest.mark.parametrize("D,causal", [(128, True), (64, False)])
def test_fwd_near_linear(lib, dev, dtype, std, cap, D, causal):
    B, H, Hk, Nq, Nk = 2, 4, 2, 517, 700
    q, k, v = qkv(B, H, Hk, Nq, Nk, D, dtype, 200 + D, std, dev)
    sc = 1.0 / math.sqrt(D)
    w = eff_window(causal, (-1, -1))
    o32, l32 = fwd(q, k, v, causal, sc, cap, None, out_f32=True)
    check_fwd(o32, l32, q, k, v, cap, None, w[0], w[1], sc, dtype, True)


# ---- 4. saturation: scaled scores of several hundred, the exponential overflows ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D,causal,window", [(128, True, (-1, -1)), (64, False, (-1, -1)), (128, False, (100, 50))])
def test_saturation(lib, dev, dtype, D, causal, window):
    from tiny_flash_attention_amd import ops

    B, H, Hk, Nq, Nk, cap = 1, 4, 2, 300, 700, 5.0
    q, k, v = qkv(B, H, Hk, Nq, Nk, D, dtype, 300 + D, 8.0, dev)
    dout = rnd((B, H, Nq, D), dtype, 304).to(dev)
    sc = 1.0 / math.sqrt(D)
    w = eff_window(causal, window)
    x = (q.double().cpu() @ k.double().cpu().repeat_interleave(H // Hk, dim=1).transpose(-1, -2)) * sc
    assert x.abs().max().item() > 200, "saturation wants scaled scores of several hundred"
    ref = ref64(q, k, v, cap, None, w[0], w[1], sc)
    o, l = fwd(q, k, v, causal, sc, cap, None, window)
    o32, l32 = fwd(q, k, v, causal, sc, cap, None, window, out_f32=True)
    check_fwd(o, l, q, k, v, cap, None, w[0], w[1], sc, dtype, False, ref=ref)
    check_fwd(o32, l32, q, k, v, cap, None, w[0], w[1], sc, dtype, True, ref=ref)
    g16 = ops.flash_attn_bwd(q, k, v, o, l, dout, causal, sc, window_size=window, softcap=cap)
    g32 = ops.flash_attn_bwd(q, k, v, o, l, dout, causal, sc, window_size=window, softcap=cap, grad_f32=True)
    torch.cuda.synchronize()
    for g in tuple(g16) + tuple(g32):
        assert not bool(torch.isnan(g).any()) and bool(torch.isfinite(g).all())
    check_bwd(g32, g16, ref_grads(q, k, v, dout, cap, None, w[0], w[1], sc), dtype, bounds=form_ref.bwd_bounds(q, k, v, o, dout, sc, softcap=cap, window=w))


# ---- 5. with alibi_slopes, with windows, with both ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("batch_slopes", [False, True])
@pytest.mark.parametrize("window,causal", [((-1, -1), False), ((-1, -1), True), ((200, 77), False), ((64, 0), True)])
def test_fwd_with_slopes(lib, dev, dtype, batch_slopes, window, causal):
    B, H, Hk, Nq, Nk, D = 2, 4, 2, 300, 700, 128
    std, cap = 2.0, 5.0
    q, k, v = qkv(B, H, Hk, Nq, Nk, D, dtype, 400, std, dev)
    sc = 1.0 / math.sqrt(D)
    slopes = (torch.stack([std_slopes(H), std_slopes(H).flip(0) * 1.5]) if batch_slopes else std_slopes(H)).to(dev)   # (B, H) / (H,)
    w = eff_window(causal, window)
    ref = ref64(q, k, v, cap, slopes, w[0], w[1], sc)
    bite_fwd(q, k, v, cap, slopes, w[0], w[1], sc, dtype, ref)
    o, l = fwd(q, k, v, causal, sc, cap, slopes, window)
    o32, l32 = fwd(q, k, v, causal, sc, cap, slopes, window, out_f32=True)
    check_fwd(o, l, q, k, v, cap, slopes, w[0], w[1], sc, dtype, False, ref=ref)
    check_fwd(o32, l32, q, k, v, cap, slopes, w[0], w[1], sc, dtype, True, ref=ref)
    # the order is cap, then bias: the bias inside the cap is a different function, far outside the bar on these inputs
    qd, kd = q.double().cpu(), k.double().cpu().repeat_interleave(H // Hk, dim=1)
    x = (qd @ kd.transpose(-1, -2)) * sc + bias64(slopes, B, H, Nq, Nk)
    s_wrong = (cap * torch.tanh(x / cap)).masked_fill(~window_mask(Nq, Nk, *w), -math.inf)
    wrong = torch.nan_to_num(torch.softmax(s_wrong, dim=-1), nan=0.0) @ v.double().cpu().repeat_interleave(H // Hk, dim=1)
    assert (wrong - ref[0]).abs().max().item() >= 10 * 1e-2, "the inputs do not tell cap-then-bias from bias-then-cap"


@pytest.mark.parametrize("window,causal", [((-1, -1), True), ((100, 50), False)])
def test_zero_slopes_give_the_bits_of_no_slopes(lib, dev, window, causal):
    from tiny_flash_attention_amd import ops

    dtype, B, H, Hk, Nq, Nk, D, cap = torch.bfloat16, 2, 4, 2, 300, 700, 64, 5.0
    q, k, v = qkv(B, H, Hk, Nq, Nk, D, dtype, 500, 2.0, dev)
    dout = rnd((B, H, Nq, D), dtype, 504).to(dev)
    sc = 1.0 / math.sqrt(D)
    for zeros in (torch.zeros(H, dtype=torch.float32, device=dev), torch.zeros(B, H, dtype=torch.float32, device=dev)):
        o0, l0 = fwd(q, k, v, causal, sc, cap, None, window)
        o1, l1 = fwd(q, k, v, causal, sc, cap, zeros, window)
        assert torch.equal(o0, o1) and torch.equal(l0, l1)
        g0 = ops.flash_attn_bwd(q, k, v, o0, l0, dout, causal, sc, window_size=window, softcap=cap)
        g1 = ops.flash_attn_bwd(q, k, v, o0, l0, dout, causal, sc, window_size=window, softcap=cap, alibi_slopes=zeros)
        torch.cuda.synchronize()
        for a, b in zip(g0, g1):
            assert torch.equal(a, b)


# ---- 6. backward against fp64 autograd, bite ------------------------------------------------------------------------------------------------
def run_bwd(dev, dtype, std, cap, window, causal, Nq, Nk, D, H, Hk, B, slopes, derivative_check):
    from tiny_flash_attention_amd import ops

    q, k, v = qkv(B, H, Hk, Nq, Nk, D, dtype, 600 + D, std, dev)
    dout = rnd((B, H, Nq, D), dtype, 604).to(dev)
    sc = 1.0 / math.sqrt(D)
    w = eff_window(causal, window)
    ref = ref_grads(q, k, v, dout, cap, slopes, w[0], w[1], sc)
    bite_bwd(ref, ref_grads(q, k, v, dout, 0.0, slopes, w[0], w[1], sc), dtype, "no cap applied")
    if derivative_check:
        bite_bwd(ref, ref_grads(q, k, v, dout, cap, slopes, w[0], w[1], sc, straight_through=True), dtype, "derivative omitted")
    o, l = ops.flash_attn_fwd(q, k, v, causal, sc, window_size=window, alibi_slopes=slopes, softcap=cap)
    g16 = ops.flash_attn_bwd(q, k, v, o, l, dout, causal, sc, window_size=window, alibi_slopes=slopes, softcap=cap)
    g32 = ops.flash_attn_bwd(q, k, v, o, l, dout, causal, sc, window_size=window, alibi_slopes=slopes, softcap=cap, grad_f32=True)
    torch.cuda.synchronize()
    check_bwd(g32, g16, ref, dtype, bounds=form_ref.bwd_bounds(q, k, v, o, dout, sc, softcap=cap, slopes=slopes, window=w))
    seen = window_mask(Nq, Nk, *w).any(dim=0)                # keys that no row sees: zero dk / dv
    if (~seen).any():
        for g in g16[1:]:
            assert bool((g[:, :, ~seen.to(dev)] == 0).all())
    g16b = ops.flash_attn_bwd(q, k, v, o, l, dout, causal, sc, window_size=window, alibi_slopes=slopes, softcap=cap)
    g32b = ops.flash_attn_bwd(q, k, v, o, l, dout, causal, sc, window_size=window, alibi_slopes=slopes, softcap=cap, grad_f32=True)
    for a, b in zip(tuple(g16) + tuple(g32), tuple(g16b) + tuple(g32b)):
        assert torch.equal(a, b)                             # two runs, the same bits


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("std", [2.0, 8.0])
@pytest.mark.parametrize("window,causal", [((-1, -1), True), ((-1, -1), False), ((100, 50), False)])
@pytest.mark.parametrize("Nq,Nk,D,H,Hk", [(300, 700, 64, 2, 2), (300, 700, 128, 4, 2), (700, 333, 128, 4, 1)])
def test_bwd_vs_fp64_bite(lib, dev, dtype, std, window, causal, Nq, Nk, D, H, Hk):
    run_bwd(dev, dtype, std, 5.0, window, causal, Nq, Nk, D, H, Hk, 1, None, False)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [64, 128])
def test_bwd_covers_the_chain_rule(lib, dev, dtype, D):
    """std 8, softcap 5, B1 H2 Nq300 Nk700 causal: a backward that omits 1 - tanh^2 (straight-through reference) is at least 10x outside every bar."""
    run_bwd(dev, dtype, 8.0, 5.0, (-1, -1), True, 300, 700, D, 2, 2, 1, None, True)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("window,causal", [((-1, -1), True), ((-1, -1), False), ((64, 0), False)])
@pytest.mark.parametrize("Nq,Nk,D,H,Hk", [(333, 700, 64, 4, 2), (700, 333, 128, 4, 1)])
def test_bwd_with_slopes(lib, dev, dtype, window, causal, Nq, Nk, D, H, Hk):
    """(B, H) slopes with different rows per batch entry under the cap: both backward launches, both gradient types."""
    B = 2
    slopes = torch.stack([std_slopes(H) * (1.0 + 2.0 * b) for b in range(B)]).flip(1).to(dev)
    run_bwd(dev, dtype, 2.0, 5.0, window, causal, Nq, Nk, D, H, Hk, B, slopes, False)


# ---- 7. flash_attn_func under autograd; flash_attn_varlen_func against per-sequence calls ------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("with_slopes", [False, True])
def test_flash_attn_func_softcap_grads(lib, dev, causal, with_slopes):
    import tiny_flash_attention_amd as tfa

    dtype, B, N, H, D, cap = torch.bfloat16, 2, 600, 4, 64, 5.0
    q, k = (rnd((B, N, H, D), dtype, s, 2.0).to(dev).requires_grad_(True) for s in (61, 62))
    v = rnd((B, N, H, D), dtype, 63).to(dev).requires_grad_(True)
    slopes = torch.stack([std_slopes(H), std_slopes(H) * 2]).to(dev) if with_slopes else None
    out = tfa.flash_attn_func(q, k, v, causal=causal, alibi_slopes=slopes, softcap=cap)
    dout = rnd((B, N, H, D), dtype, 64).to(dev)
    out.backward(dout)
    t = lambda x: x.detach().transpose(1, 2)   # noqa: E731  (B,N,H,D) -> (B,H,N,D)
    sc = 1.0 / math.sqrt(D)
    w = eff_window(causal, (-1, -1))
    ref_o, _, _ = ref64(t(q), t(k), t(v), cap, slopes, *w, sc)
    assert (t(out).double().cpu() - ref_o).abs().max().item() <= 1e-2
    ref = ref_grads(t(q), t(k), t(v), t(dout), cap, slopes, *w, sc)
    bite_bwd(ref, ref_grads(t(q), t(k), t(v), t(dout), 0.0, slopes, *w, sc), dtype, "no cap applied")
    for g, r in zip((q.grad, k.grad, v.grad), ref):
        assert bool(torch.isfinite(g).all())
        assert (t(g).double().cpu() - r).abs().max().item() <= 1e-2 * max(1.0, r.abs().max().item())
    form_ref.check_grads(None, (t(q.grad), t(k.grad), t(v.grad)), ref,
                         form_ref.bwd_bounds(t(q), t(k), t(v), t(out), t(dout), sc, softcap=cap, slopes=slopes, window=w), dtype, "flash_attn_func")
    # no grad mode: the same forward bits
    with torch.no_grad():
        out2 = tfa.flash_attn_func(q, k, v, causal=causal, alibi_slopes=slopes, softcap=cap)
    assert torch.equal(out2, out.detach())


@pytest.mark.parametrize("variant", [32, 30])
@pytest.mark.parametrize("window,causal,with_slopes", [((-1, -1), False, False), ((-1, -1), True, True), ((64, 33), False, False), ((64, 33), False, True)])
def test_varlen_softcap_vs_per_sequence(lib, dev, variant, window, causal, with_slopes):
    import tiny_flash_attention_amd as tfa
    from tiny_flash_attention_amd import ops

    dtype, H, Hk, D, cap = torch.bfloat16, 4, 2, 128, 5.0
    lq, lk = [300, 1, 517, 0, 64], [300, 90, 400, 7, 64]       # a one-row sequence, an empty one
    B = len(lq)
    cq, ck = cu_of(lq), cu_of(lk)
    tq, tk = int(cq[-1]) + 9, int(ck[-1]) + 5                 # rows past cu[B]: outside every sequence
    q = rnd((tq, H, D), dtype, 71, 2.0).to(dev).requires_grad_(True)
    k = rnd((tk, Hk, D), dtype, 72, 2.0).to(dev).requires_grad_(True)
    v = rnd((tk, Hk, D), dtype, 73).to(dev).requires_grad_(True)
    slopes = torch.stack([std_slopes(H) * (1.0 + 0.5 * b) for b in range(B)]).to(dev) if with_slopes else None
    sentinel = torch.full((tq, H, D), 7.0, dtype=dtype, device=dev)
    with forced(lib, variant):
        o_pre, lse = ops.flash_attn_varlen_fwd(q.detach(), k.detach(), v.detach(), cq.to(dev), ck.to(dev), max(lq), max(lk), causal, None,
                                               out=sentinel.clone(), window_size=window, alibi_slopes=slopes, softcap=cap)
        out = tfa.flash_attn_varlen_func(q, k, v, cq.to(dev), ck.to(dev), max(lq), max(lk), causal=causal, window_size=window, alibi_slopes=slopes,
                                         softcap=cap)
    dout = rnd((tq, H, D), dtype, 74).to(dev)
    out.backward(dout)
    torch.cuda.synchronize()
    assert bool((o_pre[int(cq[-1]):] == 7.0).all()), "rows outside every sequence must not be written"
    sc = 1.0 / math.sqrt(D)
    for b in range(B):
        q0, q1, k0, k1 = int(cq[b]), int(cq[b + 1]), int(ck[b]), int(ck[b + 1])
        if q1 == q0:
            continue
        qs = q.detach()[q0:q1].transpose(0, 1).unsqueeze(0)
        ks = k.detach()[k0:k1].transpose(0, 1).unsqueeze(0)
        vs = v.detach()[k0:k1].transpose(0, 1).unsqueeze(0)
        sl = slopes[b].contiguous() if with_slopes else None
        with forced(lib, variant):
            of, lf = ops.flash_attn_fwd(qs, ks, vs, causal, sc, window_size=window, alibi_slopes=sl, softcap=cap)
            gf = ops.flash_attn_bwd(qs, ks, vs, of, lf, dout[q0:q1].transpose(0, 1).unsqueeze(0).contiguous(), causal, sc, window_size=window,
                                    alibi_slopes=sl, softcap=cap)
        ov = out.detach()[q0:q1].transpose(0, 1).unsqueeze(0)
        assert (ov.float() - of.float()).abs().max().item() <= 1e-2
        lv = lse[:, q0:q1].unsqueeze(0)
        fin = torch.isfinite(lf)
        assert torch.equal(torch.isfinite(lv), fin)
        if fin.any():
            assert ((lv[fin] - lf[fin]).abs() / lf[fin].abs().clamp_min(1.0)).max().item() <= 1e-4
        for g, r, a, z in ((q.grad, gf[0], q0, q1), (k.grad, gf[1], k0, k1), (v.grad, gf[2], k0, k1)):
            gg = g[a:z].transpose(0, 1).unsqueeze(0).double()
            assert (gg - r.double()).abs().max().item() <= 1e-2 * max(1.0, r.double().abs().max().item())
        # ... and the sequence itself against fp64 (with the cap: a bite case wherever the sequence is long enough to have large scores)
        w = eff_window(causal, window)
        ref, _, _ = ref64(qs, ks, vs, cap, sl, *w, sc)
        assert (ov.double().cpu() - ref).abs().max().item() <= 1e-2
        dos = dout[q0:q1].transpose(0, 1).unsqueeze(0)
        form_ref.check_grads(None, tuple(g[a:z].transpose(0, 1).unsqueeze(0) for g, a, z in ((q.grad, q0, q1), (k.grad, k0, k1), (v.grad, k0, k1))),
                             form_ref.ref_grads(qs, ks, vs, dos, sc, softcap=cap, slopes=sl, window=w),
                             form_ref.bwd_bounds(qs, ks, vs, ov, dos, sc, softcap=cap, slopes=sl, window=w), dtype, f"varlen seq {b}")
        if q1 - q0 >= 300:
            un, _, _ = ref64(qs, ks, vs, 0.0, sl, *w, sc)
            assert (un - ref).abs().max().item() >= 10 * 1e-2
    for g, n in ((q.grad, int(cq[-1])), (k.grad, int(ck[-1])), (v.grad, int(ck[-1]))):
        assert bool((g[n:] == 0).all())


# ---- 8. one CUDA-graph capture of a forward + backward: softcap is a host scalar, nothing synchronises ------------------------------------------
def test_softcap_graph_capture(lib, dev):
    from tiny_flash_attention_amd import ops

    dtype, B, H, N, D, cap = torch.bfloat16, 1, 2, 384, 64, 5.0
    q, k = (rnd((B, H, N, D), dtype, s, 2.0).to(dev) for s in (81, 82))
    v, dout = rnd((B, H, N, D), dtype, 83).to(dev), rnd((B, H, N, D), dtype, 84).to(dev)
    sc = 1.0 / math.sqrt(D)

    def step():
        o, l = ops.flash_attn_fwd(q, k, v, True, sc, softcap=cap)
        return (o, l) + tuple(ops.flash_attn_bwd(q, k, v, o, l, dout, True, sc, softcap=cap))

    eager = [t.clone() for t in step()]                       # warm-up and the eager bits
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = step()
    for t in res:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(res, eager):
        assert torch.equal(a, b)
    ref = ref64(q, k, v, cap, None, -1, 0, sc)
    check_fwd(res[0], res[1], q, k, v, cap, None, -1, 0, sc, dtype, False, ref=ref)
