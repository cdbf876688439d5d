"""GPU tests of ALiBi (include/tfa.h: tfa_fwd_alibi, tfa_bwd_alibi and the varlen forms; ops alibi_slopes=).

The reference is written in this file: fp64 scores scale * q.k - slope[b,h] * |i + shift - j| (shift = Nk - Nq), FlashAttention-2's window / causal mask,
logsumexp (INCLUDING the bias), P @ v and A = P @ |v|; rows that see nothing -> out 0, lse +inf; gradients by fp64 autograd of the same expression.
Bars (include/tfa.h, "which tolerance each path guarantees"): 16-bit out |d| <= 1e-2; fp32 out |d| <= eps16 * A + 1e-6; LSE +inf exactly on rows that
see no key, elsewhere |d| <= 1e-4 * max(1, |ref|) (with Nq > Nk and no causal mask the LSE itself is of the order of slope * (Nq - Nk)); gradients
max|d| <= 1e-2 * max(1, max|ref|) (16 bit) and <= 8 * eps16 * max(1, max|ref|) (fp32), finite, deterministic.  Steep slopes (8x the standard ones) put
nearly all of a row's weight on one key, |out| approaches |v| and bf16's own output rounding reaches 7.6e-3: those cases assert the fp32-out bound and
the LSE only.
  1. alibi_slopes=None: the bits of today's calls;  2. forward vs fp64 (both edges, Nq != Nk, variants, dtypes, head dims, GQA, (H,) / (B,H), slope 0);
  3. steep slopes at N = 2048 (the first tile visited is the farthest);  4. slopes with windows;  5. backward vs fp64 autograd;
  6. flash_attn_func;  7. flash_attn_varlen_func against per-sequence calls;  8. one CUDA-graph capture, slopes overwritten in place.
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


def scores64(q64, k64, slopes, left, right, sc):
    B, H, Nq, _ = q64.shape
    Nk = k64.shape[2]
    s = (q64 @ k64.transpose(-1, -2)) * sc + bias64(slopes, B, H, Nq, Nk)
    m = window_mask(Nq, Nk, left, right)
    return s.masked_fill(~m, -math.inf), m


def ref64(q, k, v, slopes, left, right, sc):
    """q (B,H,Nq,D), k / v (B,Hk,Nk,D) -> out64, lse64, A (sum_j P |v|), on the CPU in fp64."""
    q, k, v = q.double().cpu(), k.double().cpu(), v.double().cpu()
    G = q.shape[1] // k.shape[1]
    k, v = k.repeat_interleave(G, dim=1), v.repeat_interleave(G, dim=1)
    s, m = scores64(q, k, slopes, left, right, sc)
    lse = torch.logsumexp(s, dim=-1)
    p = torch.nan_to_num(torch.exp(s - lse.unsqueeze(-1)), nan=0.0)
    empty = ~m.any(dim=-1)
    lse = lse.masked_fill(empty.view(1, 1, -1).expand_as(lse), math.inf)
    return p @ v, lse, p @ v.abs()


def ref_grads(q, k, v, dout, slopes, left, right, sc):
    q64, k64, v64 = (t.double().cpu().requires_grad_(True) for t in (q, k, v))
    G = q.shape[1] // k.shape[1]
    kk, vv = k64.repeat_interleave(G, dim=1), v64.repeat_interleave(G, dim=1)
    s, _ = scores64(q64, kk, slopes, left, right, sc)
    p = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)
    (p @ vv).backward(dout.double().cpu())
    return q64.grad, k64.grad, v64.grad


def check_fwd(out, lse, q, k, v, slopes, left, right, sc, dtype, f32, out16=True):
    ref, lref, A = ref64(q, k, v, slopes, left, right, sc)
    o = out.double().cpu()
    if f32:
        eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
        ex = ((o - ref).abs() - (eps * A + 1e-6)).max().item()
        print(f"fp32 out: max(|d| - (eps16 * A + 1e-6)) = {ex:.3e}")
        assert ex <= 0, f"fp32 out exceeds eps16 * A + 1e-6 by {ex:.3e}"
    elif out16:
        err = (o - ref).abs().max().item()
        print(f"16-bit out: max|d| = {err:.3e}")
        assert err <= 1e-2, f"out: max|d| = {err:.3e}"
    l = lse.double().cpu()
    inf = torch.isinf(lref)
    assert torch.equal(torch.isinf(l), inf) and bool((l[inf] > 0).all()), "lse must be +inf exactly on rows that see no key"
    if (~inf).any():
        e = ((l[~inf] - lref[~inf]).abs() / lref[~inf].abs().clamp_min(1.0)).max().item()
        print(f"lse: max|d| / max(1, |ref|) = {e:.3e} (max|ref| = {lref[~inf].abs().max().item():.1f})")
        assert e <= 1e-4, f"lse: max|d| / max(1, |ref|) = {e:.3e}"
    assert bool((o[inf.unsqueeze(-1).expand_as(o)] == 0).all()), "rows that see no key must be 0"


def check_bwd(g32, g16, q, k, v, dout, slopes, left, right, sc, dtype, out=None):
    ref = ref_grads(q, k, v, dout, slopes, left, right, sc)
    if out is not None:     # element by element: (B1) / (B2) with the bound of tests/form_ref.py (out: the 16-bit O the forward stored)
        form_ref.check_grads(g32, g16, ref, form_ref.bwd_bounds(q, k, v, out, dout, sc, slopes=slopes, window=(left, right)), dtype, f"alibi {(left, right)}")
    eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    for name, a32, a16, r in zip(("dq", "dk", "dv"), g32, g16, ref):
        a32c, a16c = a32.double().cpu(), a16.double().cpu()
        assert bool(torch.isfinite(a16c).all()) and bool(torch.isfinite(a32c).all()), name
        scale = max(1.0, r.abs().max().item())
        e16, e32 = (a16c - r).abs().max().item(), (a32c - r).abs().max().item()
        print(f"{name}: 16-bit max|d| = {e16:.3e}, fp32 max|d| = {e32:.3e}, max|ref| = {r.abs().max().item():.3e}")
        assert e16 <= 1e-2 * scale, f"{name}: {e16:.3e}"
        assert e32 <= 8 * eps * scale, f"{name} fp32: {e32:.3e}"


def fwd(q, k, v, causal, sc, slopes, window=(-1, -1), out_f32=False):
    from tiny_flash_attention_amd import ops

    o, l = ops.flash_attn_fwd(q, k, v, causal, sc, out_f32=out_f32, window_size=window, alibi_slopes=slopes)
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


# ---- 1. alibi_slopes=None is today's call, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [(-1, -1), (100, 0)])
@pytest.mark.parametrize("causal", [False, True])
def test_none_is_todays_call_fixed(lib, dev, window, causal):
    from tiny_flash_attention_amd import ops

    dtype, B, H, Nq, Nk, D = torch.bfloat16, 2, 4, 300, 700, 64
    q, k, v = (rnd((B, H, n, D), dtype, s).to(dev) for s, n in ((1, Nq), (2, Nk), (3, Nk)))
    dout = rnd((B, H, Nq, D), dtype, 4).to(dev)
    sc = 1.0 / math.sqrt(D)
    o0, l0 = ops.flash_attn_fwd(q, k, v, causal, sc, window_size=window)
    o1, l1 = ops.flash_attn_fwd(q, k, v, causal, sc, window_size=window, alibi_slopes=None)
    assert torch.equal(o0, o1) and torch.equal(l0, l1)
    g0 = ops.flash_attn_bwd(q, k, v, o0, l0, dout, causal, sc, window_size=window)
    g1 = ops.flash_attn_bwd(q, k, v, o0, l0, dout, causal, sc, window_size=window, alibi_slopes=None)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)


@pytest.mark.parametrize("window", [(-1, -1), (64, 0)])
def test_none_is_todays_call_varlen(lib, dev, window):
    from tiny_flash_attention_amd import ops

    dtype, H, D = torch.bfloat16, 4, 64
    lq, lk = [100, 200, 37], [150, 200, 90]
    cq, ck = cu_of(lq).to(dev), cu_of(lk).to(dev)
    q, k, v = rnd((sum(lq), H, D), dtype, 5).to(dev), rnd((sum(lk), H, D), dtype, 6).to(dev), rnd((sum(lk), H, D), dtype, 7).to(dev)
    dout = rnd((sum(lq), H, D), dtype, 8).to(dev)
    o0, l0 = ops.flash_attn_varlen_fwd(q, k, v, cq, ck, 200, 200, True, None, window_size=window)
    o1, l1 = ops.flash_attn_varlen_fwd(q, k, v, cq, ck, 200, 200, True, None, window_size=window, alibi_slopes=None)
    assert torch.equal(o0, o1) and torch.equal(l0, l1)
    g0 = ops.flash_attn_varlen_bwd(q, k, v, o0, l0, dout, cq, ck, 200, 200, True, None, window_size=window)
    g1 = ops.flash_attn_varlen_bwd(q, k, v, o0, l0, dout, cq, ck, 200, 200, True, None, window_size=window, alibi_slopes=None)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)


# ---- 2. forward against fp64 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("Nq,Nk", [(700, 700), (300, 900), (900, 333)])
@pytest.mark.parametrize("variant", [30, 32])
def test_fwd_vs_fp64(lib, dev, causal, Nq, Nk, variant):
    dtype, D, B, H = torch.bfloat16, 128, 2, 4
    q, k, v = rnd((B, H, Nq, D), dtype, 11).to(dev), rnd((B, H, Nk, D), dtype, 12).to(dev), rnd((B, H, Nk, D), dtype, 13).to(dev)
    sc = 1.0 / math.sqrt(D)
    slopes = torch.stack([std_slopes(H), std_slopes(H).flip(0) * 1.5]).to(dev)          # (B, H), different rows per batch entry
    w = eff_window(causal, (-1, -1))
    with forced(lib, variant):
        o, l = fwd(q, k, v, causal, sc, slopes)
        o32, l32 = fwd(q, k, v, causal, sc, slopes, out_f32=True)
    check_fwd(o, l, q, k, v, slopes, w[0], w[1], sc, dtype, False)
    check_fwd(o32, l32, q, k, v, slopes, w[0], w[1], sc, dtype, True)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [40, 64, 96, 128])
@pytest.mark.parametrize("causal", [False, True])
def test_fwd_dtypes_dims_gqa(lib, dev, dtype, D, causal):
    B, H, Hk, Nq, Nk = 2, 4, 2, 517, 517
    q, k, v = rnd((B, H, Nq, D), dtype, 21).to(dev), rnd((B, Hk, Nk, D), dtype, 22).to(dev), rnd((B, Hk, Nk, D), dtype, 23).to(dev)
    sc = 1.0 / math.sqrt(D)
    slopes = torch.tensor([0.5, 0.0, 0.0625, 0.01], dtype=torch.float32, device=dev)     # (H,): four distinct slopes, one of them 0
    w = eff_window(causal, (-1, -1))
    o, l = fwd(q, k, v, causal, sc, slopes)
    o32, l32 = fwd(q, k, v, causal, sc, slopes, out_f32=True)
    check_fwd(o, l, q, k, v, slopes, w[0], w[1], sc, dtype, False)
    check_fwd(o32, l32, q, k, v, slopes, w[0], w[1], sc, dtype, True)
    # the head with slope 0 agrees with the call without slopes within the bars (other kernels: not in bits)
    o0, l0 = fwd(q, k, v, causal, sc, None)
    e0 = (o[:, 1].float() - o0[:, 1].float()).abs().max().item()
    fin = torch.isfinite(l0[:, 1])
    el = ((l[:, 1][fin] - l0[:, 1][fin]).abs() / l0[:, 1][fin].abs().clamp_min(1.0)).max().item()
    print(f"slope-0 head vs no slopes: out max|d| = {e0:.3e}, lse max|d| / max(1, |l0|) = {el:.3e}")
    assert e0 <= 1e-2
    assert el <= 1e-4


# ---- 3. steep slopes: the bias dominates, the first tile visited is the farthest ------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("variant", [30, 32])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_fwd_steep_slopes(lib, dev, causal, variant, dtype):
    D, B, H, N = 128, 1, 8, 2048
    q, k, v = (rnd((B, H, N, D), dtype, s).to(dev) for s in (31, 32, 33))
    sc = 1.0 / math.sqrt(D)
    slopes = std_slopes(H, 8.0).to(dev)
    w = eff_window(causal, (-1, -1))
    with forced(lib, variant):
        o32, l = fwd(q, k, v, causal, sc, slopes, out_f32=True)
    check_fwd(o32, l, q, k, v, slopes, w[0], w[1], sc, dtype, True)


# ---- 4. slopes together with windows -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window,causal", [((64, 0), False), ((300, 0), False), ((128, 128), False), ((-1, 64), False), ((64, -1), False), ((200, 77), True)])
@pytest.mark.parametrize("Nq,Nk", [(700, 700), (300, 900), (900, 333)])
def test_fwd_slopes_with_windows(lib, dev, window, causal, Nq, Nk):
    dtype, D, B, H = torch.bfloat16, 128, 1, 4
    q, k, v = rnd((B, H, Nq, D), dtype, 41).to(dev), rnd((B, H, Nk, D), dtype, 42).to(dev), rnd((B, H, Nk, D), dtype, 43).to(dev)
    sc = 1.0 / math.sqrt(D)
    slopes = std_slopes(H).to(dev)
    w = eff_window(causal, window)
    o, l = fwd(q, k, v, causal, sc, slopes, window)
    o32, l32 = fwd(q, k, v, causal, sc, slopes, window, out_f32=True)
    check_fwd(o, l, q, k, v, slopes, w[0], w[1], sc, dtype, False)
    check_fwd(o32, l32, q, k, v, slopes, w[0], w[1], sc, dtype, True)


# ---- 5. backward against fp64 autograd ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("window,causal", [((-1, -1), True), ((-1, -1), False), ((64, 0), False), ((128, 128), False)])
@pytest.mark.parametrize("Nq,Nk,D,H,Hk", [(640, 640, 128, 2, 2), (333, 700, 64, 4, 2), (700, 333, 128, 4, 1)])
def test_bwd_vs_fp64(lib, dev, dtype, window, causal, Nq, Nk, D, H, Hk):
    run_bwd_vs_fp64(dev, dtype, window, causal, Nq, Nk, D, H, Hk, 1)


@pytest.mark.parametrize("window,causal", [((-1, -1), True), ((-1, -1), False), ((64, 0), False)])
@pytest.mark.parametrize("Nq,Nk,D,H,Hk", [(333, 700, 64, 4, 2), (700, 333, 128, 4, 1)])
def test_bwd_batch_slopes_vs_fp64(lib, dev, window, causal, Nq, Nk, D, H, Hk):
    """(B, H) slopes with different rows per batch entry: the batch index of the slopes in both backward launches, at the fp32-gradient bar."""
    run_bwd_vs_fp64(dev, torch.bfloat16, window, causal, Nq, Nk, D, H, Hk, 2)


def run_bwd_vs_fp64(dev, dtype, window, causal, Nq, Nk, D, H, Hk, B):
    from tiny_flash_attention_amd import ops

    q, k, v = rnd((B, H, Nq, D), dtype, 51).to(dev), rnd((B, Hk, Nk, D), dtype, 52).to(dev), rnd((B, Hk, Nk, D), dtype, 53).to(dev)
    dout = rnd((B, H, Nq, D), dtype, 54).to(dev)
    sc = 1.0 / math.sqrt(D)
    slopes = (std_slopes(H) if B == 1 else torch.stack([std_slopes(H) * (1.0 + 2.0 * b) for b in range(B)]).flip(1 if B > 1 else 0)).to(dev)
    w = eff_window(causal, window)
    o, l = ops.flash_attn_fwd(q, k, v, causal, sc, window_size=window, alibi_slopes=slopes)
    g16 = ops.flash_attn_bwd(q, k, v, o, l, dout, causal, sc, window_size=window, alibi_slopes=slopes)
    g32 = ops.flash_attn_bwd(q, k, v, o, l, dout, causal, sc, window_size=window, alibi_slopes=slopes, grad_f32=True)
    torch.cuda.synchronize()
    check_bwd(g32, g16, q, k, v, dout, slopes, w[0], w[1], sc, dtype, out=o)
    seen = window_mask(Nq, Nk, *w).any(dim=0)                # keys that no row sees: zero dk / dv
    if (~seen).any():
        for g in g16[1:]:
            assert bool((g[:, :, ~seen.to(dev)] == 0).all())
    g16b = ops.flash_attn_bwd(q, k, v, o, l, dout, causal, sc, window_size=window, alibi_slopes=slopes)
    for a, b in zip(g16, g16b):
        assert torch.equal(a, b)                             # deterministic


# ---- 6. flash_attn_func -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
def test_flash_attn_func_alibi_grads(lib, dev, causal):
    import tiny_flash_attention_amd as tfa

    dtype, B, N, H, D = torch.bfloat16, 2, 600, 4, 64
    q, k, v = (rnd((B, N, H, D), dtype, s).to(dev).requires_grad_(True) for s in (61, 62, 63))
    slopes = torch.stack([std_slopes(H), std_slopes(H) * 2]).to(dev)
    assert not slopes.requires_grad
    out = tfa.flash_attn_func(q, k, v, causal=causal, alibi_slopes=slopes)
    dout = rnd((B, N, H, D), dtype, 64).to(dev)
    out.backward(dout)
    assert slopes.grad is None
    t = lambda x: x.detach().transpose(1, 2)   # noqa: E731  (B,N,H,D) -> (B,H,N,D)
    sc = 1.0 / math.sqrt(D)
    w = eff_window(causal, (-1, -1))
    ref_o, _, _ = ref64(t(q), t(k), t(v), slopes, *w, sc)
    assert (t(out).double().cpu() - ref_o).abs().max().item() <= 1e-2
    ref = ref_grads(t(q), t(k), t(v), t(dout), slopes, *w, sc)
    for g, r in zip((q.grad, k.grad, v.grad), ref):
        assert bool(torch.isfinite(g).all())
        assert (t(g).double().cpu() - r).abs().max().item() <= 1e-2 * max(1.0, r.abs().max().item())
    form_ref.check_grads(None, (t(q.grad), t(k.grad), t(v.grad)), ref, form_ref.bwd_bounds(t(q), t(k), t(v), t(out), t(dout), sc, slopes=slopes, window=w), dtype,
                         "flash_attn_func")
    # slopes that require grad get none
    s2 = slopes.clone().requires_grad_(True)
    q2 = q.detach().clone().requires_grad_(True)
    tfa.flash_attn_func(q2, k.detach(), v.detach(), causal=causal, alibi_slopes=s2).backward(dout)
    assert s2.grad is None and torch.equal(q2.grad, q.grad)


# ---- 7. flash_attn_varlen_func against per-sequence fixed-length calls ----------------------------------------------------------------------
@pytest.mark.parametrize("variant", [32, 30])
@pytest.mark.parametrize("window,causal", [((-1, -1), False), ((-1, -1), True), ((64, 33), False)])
def test_varlen_alibi_vs_per_sequence(lib, dev, variant, window, causal):
    import tiny_flash_attention_amd as tfa
    from tiny_flash_attention_amd import ops

    dtype, H, Hk, D = torch.bfloat16, 4, 2, 128
    lq, lk = [300, 1, 517, 0, 64], [300, 90, 400, 7, 64]
    B = len(lq)
    cq, ck = cu_of(lq), cu_of(lk)
    tq, tk = int(cq[-1]) + 9, int(ck[-1]) + 5                 # rows past cu[B]: outside every sequence
    q = rnd((tq, H, D), dtype, 71).to(dev).requires_grad_(True)
    k = rnd((tk, Hk, D), dtype, 72).to(dev).requires_grad_(True)
    v = rnd((tk, Hk, D), dtype, 73).to(dev).requires_grad_(True)
    slopes = torch.stack([std_slopes(H) * (1.0 + 0.5 * b) for b in range(B)]).to(dev)      # (B, H): a row per sequence
    sentinel = torch.full((tq, H, D), 7.0, dtype=dtype, device=dev)
    with forced(lib, variant):
        o_pre, lse = ops.flash_attn_varlen_fwd(q.detach(), k.detach(), v.detach(), cq.to(dev), ck.to(dev), max(lq), max(lk), causal, None,
                                               out=sentinel.clone(), window_size=window, alibi_slopes=slopes)
        out = tfa.flash_attn_varlen_func(q, k, v, cq.to(dev), ck.to(dev), max(lq), max(lk), causal=causal, window_size=window, alibi_slopes=slopes)
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
        if k1 == k0:
            assert bool((out.detach()[q0:q1] == 0).all())
            continue
        with forced(lib, variant):
            of, lf = ops.flash_attn_fwd(qs, ks, vs, causal, sc, window_size=window, alibi_slopes=slopes[b].contiguous())
            gf = ops.flash_attn_bwd(qs, ks, vs, of, lf, dout[q0:q1].transpose(0, 1).unsqueeze(0).contiguous(), causal, sc, window_size=window,
                                    alibi_slopes=slopes[b].contiguous())
        ov = out.detach()[q0:q1].transpose(0, 1).unsqueeze(0)
        assert (ov.float() - of.float()).abs().max().item() <= 1e-2
        for g, r, a, z in ((q.grad, gf[0], q0, q1), (k.grad, gf[1], k0, k1), (v.grad, gf[2], k0, k1)):
            gg = g[a:z].transpose(0, 1).unsqueeze(0).double()
            assert (gg - r.double()).abs().max().item() <= 1e-2 * max(1.0, r.double().abs().max().item())
        # ... and the sequence itself against fp64
        w = eff_window(causal, window)
        ref, _, _ = ref64(qs, ks, vs, slopes[b], *w, sc)
        assert (ov.double().cpu() - ref).abs().max().item() <= 1e-2
        dos = dout[q0:q1].transpose(0, 1).unsqueeze(0)
        form_ref.check_grads(None, tuple(g[a:z].transpose(0, 1).unsqueeze(0) for g, a, z in ((q.grad, q0, q1), (k.grad, k0, k1), (v.grad, k0, k1))),
                             form_ref.ref_grads(qs, ks, vs, dos, sc, slopes=slopes[b], window=w),
                             form_ref.bwd_bounds(qs, ks, vs, ov, dos, sc, slopes=slopes[b], window=w), dtype, f"varlen seq {b}")
    for g, n in ((q.grad, int(cq[-1])), (k.grad, int(ck[-1])), (v.grad, int(ck[-1]))):
        assert bool((g[n:] == 0).all())


# ---- 8. one CUDA-graph capture: the slopes are read on the device ------------------------------------------------------------------------------
def test_varlen_alibi_graph_capture(lib, dev):
    from tiny_flash_attention_amd import ops

    dtype, H, D = torch.bfloat16, 2, 64
    tq = 600
    q, k, v = (rnd((tq, H, D), dtype, s).to(dev) for s in (81, 82, 83))
    cq = cu_of([100, 200, 300]).to(dev)
    ck = cu_of([100, 200, 300]).to(dev)
    slopes = torch.stack([std_slopes(H)] * 3).to(dev)
    out = torch.zeros((tq, H, D), dtype=dtype, device=dev)
    ops.flash_attn_varlen_fwd(q, k, v, cq, ck, 300, 300, True, None, out=out, return_lse=False, alibi_slopes=slopes)   # warm-up
    torch.cuda.synchronize()
    eager0 = out.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.flash_attn_varlen_fwd(q, k, v, cq, ck, 300, 300, True, None, out=out, return_lse=False, alibi_slopes=slopes)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager0)
    slopes.copy_(torch.tensor([[0.3, 0.0], [1.0, 0.02], [-0.01, 0.5]], dtype=torch.float32))   # in place: zero and negative values are legal
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    eager1, _ = ops.flash_attn_varlen_fwd(q, k, v, cq, ck, 300, 300, True, None, alibi_slopes=slopes)
    torch.cuda.synchronize()
    assert torch.equal(out, eager1) and not torch.equal(out, eager0)
