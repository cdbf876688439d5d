"""GPU tests of local (sliding-window) attention (include/tfa.h: tfa_fwd_local, tfa_bwd_local and the varlen forms; ops window_size=).

The reference here is written in this file: fp64 attention with FlashAttention-2's window mask (key j visible to row i iff
i + shift - left <= j <= i + shift + right, shift = Nk - Nq, -1 unbounded), rows that see nothing -> out 0, lse +inf.
  1. (-1, -1) / (-1, 0) give the bits of the full / causal call, forward and backward;
  2. forward against fp64 with the header's bars: atol 1e-2 on 16-bit out, eps16 * A + 1e-6 on fp32 out (A = sum_j P |v|), LSE within 1e-4 and +inf
     exactly where a row sees nothing — windows on both edges, Nq == / < / > Nk, ragged N, il4 and il8 forced, both dtypes, D 40 / 64 / 96 / 128, GQA;
  3. a peaked row whose dominant key lies inside its window but outside the first key tile the pass visits;
  4. backward against fp64 autograd of the masked reference (max|d| <= 1e-2 * max(1, max|ref|) and an fp32-gradient bound eps16 * |ref|-scale),
     GQA sums, zero dk / dv for keys no row sees, determinism;
  5. flash_attn_func(window_size=) gradients, flash_attn_varlen_func with a window against per-sequence fixed-length calls, isolation of rows outside
     every sequence, one CUDA-graph capture of a varlen local call.
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


def ref64(q, k, v, left, right, sc):
    """q (B,H,Nq,D), k / v (B,Hk,Nk,D), any float dtype -> out64, lse64, A (sum_j P |v|), all on the CPU in fp64."""
    q, k, v = q.double().cpu(), k.double().cpu(), v.double().cpu()
    G = q.shape[1] // k.shape[1]
    k = k.repeat_interleave(G, dim=1)
    v = v.repeat_interleave(G, dim=1)
    m = window_mask(q.shape[2], k.shape[2], left, right)
    s = (q @ k.transpose(-1, -2)) * sc
    s = s.masked_fill(~m, -math.inf)
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.unsqueeze(-1))
    p = torch.nan_to_num(p, nan=0.0)
    empty = ~m.any(dim=-1)
    lse = lse.masked_fill(empty.view(1, 1, -1).expand_as(lse), math.inf)
    return p @ v, lse, p @ v.abs()


def ref_grads(q, k, v, dout, left, right, sc):
    """fp64 autograd of the masked reference (GQA: dk / dv summed over each K/V head's query heads)."""
    q64, k64, v64 = (t.double().cpu().requires_grad_(True) for t in (q, k, v))
    G = q.shape[1] // k.shape[1]
    kk, vv = k64.repeat_interleave(G, dim=1), v64.repeat_interleave(G, dim=1)
    m = window_mask(q.shape[2], k.shape[2], left, right)
    s = ((q64 @ kk.transpose(-1, -2)) * sc).masked_fill(~m, -math.inf)
    p = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)
    (p @ vv).backward(dout.double().cpu())
    return q64.grad, k64.grad, v64.grad


def check_fwd(out, lse, q, k, v, left, right, sc, dtype, f32):
    ref, lref, A = ref64(q, k, v, left, right, sc)
    o = out.double().cpu()
    if f32:
        eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
        ex = ((o - ref).abs() - (eps * A + 1e-6)).max().item()
        assert ex <= 0, f"fp32 out exceeds eps16 * A + 1e-6 by {ex:.3e}"
    else:
        err = (o - ref).abs().max().item()
        assert err <= 1e-2, f"out: max|d| = {err:.3e}"
    l = lse.double().cpu()
    inf = torch.isinf(lref)
    assert torch.equal(torch.isinf(l), inf) and bool((l[inf] > 0).all()), "lse must be +inf exactly on rows that see no key"
    if (~inf).any():
        e = (l[~inf] - lref[~inf]).abs().max().item()
        assert e <= 1e-4, f"lse: max|d| = {e:.3e}"
    assert bool((o[inf.unsqueeze(-1).expand_as(o)] == 0).all()), "rows that see no key must be 0"


def fwd(q, k, v, causal, sc, window, out_f32=False):
    from tiny_flash_attention_amd import ops

    o, l = ops.flash_attn_fwd(q, k, v, causal, sc, out_f32=out_f32, window_size=window)
    torch.cuda.synchronize()
    return o, l


def forced(lib, variant):
    class _F:
        def __enter__(self):
            lib.set_variant(variant)

        def __exit__(self, *a):
            lib.set_variant(-1)
    return _F()


# ---- 1. full / causal windows are the existing calls, bit for bit ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,H,Nq,Nk,D", [(2, 4, 512, 512, 128), (1, 8, 300, 700, 64), (2, 2, 1024, 1024, 96)])
def test_full_and_causal_windows_same_bits(lib, dev, dtype, B, H, Nq, Nk, D):
    from tiny_flash_attention_amd import ops

    q, k, v = (rnd((B, H, n, D), dtype, s).to(dev) for s, n in ((1, Nq), (2, Nk), (3, Nk)))
    dout = rnd((B, H, Nq, D), dtype, 4).to(dev)
    sc = 1.0 / math.sqrt(D)
    for window, causal in (((-1, -1), False), ((-1, 0), True)):
        o0, l0 = ops.flash_attn_fwd(q, k, v, causal, sc)
        o1, l1 = ops.flash_attn_fwd(q, k, v, False, sc, window_size=window)
        assert torch.equal(o0, o1) and torch.equal(l0, l1), window
        g0 = ops.flash_attn_bwd(q, k, v, o0, l0, dout, causal, sc)
        g1 = ops.flash_attn_bwd(q, k, v, o0, l0, dout, False, sc, window_size=window)
        for a, b in zip(g0, g1):
            assert torch.equal(a, b), window


# ---- 2. forward against fp64 ------------------------------------------------------------------------------------------------------------
WINDOWS = [(0, 0), (1, 0), (63, 0), (64, 0), (65, 0), (255, 0), (256, 0), (1000, 0), (10 ** 6, 0), (128, 128), (0, 300), (-1, 64), (64, -1)]


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("Nq,Nk", [(700, 700), (300, 900), (900, 333)])
@pytest.mark.parametrize("variant", [30, 32])
def test_fwd_windows_vs_fp64(lib, dev, window, Nq, Nk, variant):
    dtype, D, B, H = torch.bfloat16, 128, 1, 2
    q, k, v = rnd((B, H, Nq, D), dtype, 11).to(dev), rnd((B, H, Nk, D), dtype, 12).to(dev), rnd((B, H, Nk, D), dtype, 13).to(dev)
    sc = 1.0 / math.sqrt(D)
    with forced(lib, variant):
        o, l = fwd(q, k, v, False, sc, window)
        o32, _ = fwd(q, k, v, False, sc, window, out_f32=True)
    check_fwd(o, l, q, k, v, window[0], window[1], sc, dtype, False)
    check_fwd(o32, l, q, k, v, window[0], window[1], sc, dtype, True)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [40, 64, 96, 128])
@pytest.mark.parametrize("window", [(100, 0), (37, 90), (300, 0)])
@pytest.mark.parametrize("variant", [-1, 30])
def test_fwd_dtypes_dims_gqa(lib, dev, dtype, D, window, variant):
    B, H, Hk, Nq, Nk = 2, 4, 2, 517, 517
    q, k, v = rnd((B, H, Nq, D), dtype, 21).to(dev), rnd((B, Hk, Nk, D), dtype, 22).to(dev), rnd((B, Hk, Nk, D), dtype, 23).to(dev)
    sc = 1.0 / math.sqrt(D)
    with forced(lib, variant):
        o, l = fwd(q, k, v, False, sc, window)
        o32, _ = fwd(q, k, v, False, sc, window, out_f32=True)
    check_fwd(o, l, q, k, v, window[0], window[1], sc, dtype, False)
    check_fwd(o32, l, q, k, v, window[0], window[1], sc, dtype, True)


def test_fwd_causal_flag_forces_right_zero(lib, dev):
    dtype, D = torch.bfloat16, 64
    q, k, v = (rnd((1, 2, 640, D), dtype, s).to(dev) for s in (31, 32, 33))
    sc = 0.125
    o, l = fwd(q, k, v, True, sc, (200, 77))
    check_fwd(o, l, q, k, v, 200, 0, sc, dtype, False)


def test_fwd_peaked_row_outside_first_tile(lib, dev):
    """Each row's dominant key lies inside its window but outside the first key tile its block visits: the lazy rule re-bases on it (P of
    the dominant key rounds as 1), so the fp32 output stays inside eps16 * A of fp64."""
    dtype, D, N, left = torch.bfloat16, 128, 2048, 700
    q = rnd((1, 2, N, D), dtype, 41)
    k = rnd((1, 2, N, D), dtype, 42)
    v = rnd((1, 2, N, D), dtype, 43)
    qd = q.float()
    for i in range(0, N, 7):                          # key i - 5 (inside the window, far from the block's first tile) aligned with row i, scaled up
        j = max(i - 5, 0)
        k[0, :, j] = (qd[0, :, i] * 6.0).to(dtype)
    q, k, v = q.to(dev), k.to(dev), v.to(dev)
    sc = 1.0 / math.sqrt(D)
    for variant in (30, 32):
        with forced(lib, variant):
            o32, l = fwd(q, k, v, False, sc, (left, 0), out_f32=True)
        check_fwd(o32, l, q, k, v, left, 0, sc, dtype, True)


# ---- 4. backward ------------------------------------------------------------------------------------------------------------------------
def check_bwd(g32, g16, q, k, v, dout, left, right, sc, dtype, out=None):
    ref = ref_grads(q, k, v, dout, left, right, sc)
    if out is not None:     # element by element: (B1) / (B2) with the bound of tests/form_ref.py (out: the 16-bit O the forward stored)
        form_ref.check_grads(g32, g16, ref, form_ref.bwd_bounds(q, k, v, out, dout, sc, window=(left, right)), dtype, f"window {(left, right)}")
    for name, a32, a16, r in zip(("dq", "dk", "dv"), g32, g16, ref):
        a32c, a16c = a32.double().cpu(), a16.double().cpu()
        assert bool(torch.isfinite(a16c).all()), name
        scale = max(1.0, r.abs().max().item())
        assert (a16c - r).abs().max().item() <= 1e-2 * scale, f"(B3) {name}: {(a16c - r).abs().max().item():.3e}"
        eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
        assert (a32c - r).abs().max().item() <= 8 * eps * scale, f"{name} fp32: {(a32c - r).abs().max().item():.3e}"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("window", [(0, 0), (64, 0), (129, 0), (300, 0), (128, 128), (0, 300), (-1, 64), (64, -1)])
@pytest.mark.parametrize("Nq,Nk,D,H,Hk", [(640, 640, 128, 2, 2), (333, 700, 64, 4, 2), (700, 333, 128, 4, 1)])
def test_bwd_windows_vs_fp64(lib, dev, dtype, window, Nq, Nk, D, H, Hk):
    from tiny_flash_attention_amd import ops

    B = 1
    q, k, v = rnd((B, H, Nq, D), dtype, 51).to(dev), rnd((B, Hk, Nk, D), dtype, 52).to(dev), rnd((B, Hk, Nk, D), dtype, 53).to(dev)
    dout = rnd((B, H, Nq, D), dtype, 54).to(dev)
    sc = 1.0 / math.sqrt(D)
    o, l = ops.flash_attn_fwd(q, k, v, False, sc, window_size=window)
    g16 = ops.flash_attn_bwd(q, k, v, o, l, dout, False, sc, window_size=window)
    g32 = ops.flash_attn_bwd(q, k, v, o, l, dout, False, sc, window_size=window, grad_f32=True)
    torch.cuda.synchronize()
    check_bwd(g32, g16, q, k, v, dout, window[0], window[1], sc, dtype, out=o)
    # keys that no row sees: zero dk / dv; determinism: a second run gives the same bits
    seen = window_mask(Nq, Nk, *window).any(dim=0)
    if (~seen).any():
        for g in g16[1:]:
            assert bool((g[:, :, ~seen.to(dev)] == 0).all())
    g16b = ops.flash_attn_bwd(q, k, v, o, l, dout, False, sc, window_size=window)
    for a, b in zip(g16, g16b):
        assert torch.equal(a, b)


# ---- 5. autograd, varlen, graphs --------------------------------------------------------------------------------------------------------
def test_flash_attn_func_window_grads(lib, dev):
    import tiny_flash_attention_amd as tfa

    dtype, B, N, H, D, window = torch.bfloat16, 2, 600, 4, 64, (150, 20)
    q, k, v = (rnd((B, N, H, D), dtype, s).to(dev).requires_grad_(True) for s in (61, 62, 63))
    out = tfa.flash_attn_func(q, k, v, causal=False, window_size=window)
    dout = rnd((B, N, H, D), dtype, 64).to(dev)
    out.backward(dout)
    t = lambda x: x.detach().transpose(1, 2)   # noqa: E731  (B,N,H,D) -> (B,H,N,D)
    sc = 1.0 / math.sqrt(D)
    ref_o, _, _ = ref64(t(q), t(k), t(v), *window, sc)
    assert (t(out).double().cpu() - ref_o).abs().max().item() <= 1e-2
    ref = ref_grads(t(q), t(k), t(v), t(dout), *window, sc)
    for g, r in zip((q.grad, k.grad, v.grad), ref):
        assert (t(g).double().cpu() - r).abs().max().item() <= 1e-2 * max(1.0, r.abs().max().item())
    form_ref.check_grads(None, (t(q.grad), t(k.grad), t(v.grad)), ref, form_ref.bwd_bounds(t(q), t(k), t(v), t(out), t(dout), sc, window=window), dtype, "flash_attn_func")


def cu_of(lens):
    c = [0]
    for n in lens:
        c.append(c[-1] + n)
    return torch.tensor(c, dtype=torch.int32)


@pytest.mark.parametrize("variant", [32, 30])
@pytest.mark.parametrize("window", [(100, 0), (64, 33), (-1, 50)])
def test_varlen_window_vs_per_sequence(lib, dev, variant, window):
    import tiny_flash_attention_amd as tfa
    from tiny_flash_attention_amd import ops

    dtype, H, Hk, D = torch.bfloat16, 4, 2, 128
    lq, lk = [300, 1, 517, 0, 64], [300, 90, 400, 7, 64]
    cq, ck = cu_of(lq), cu_of(lk)
    tq, tk = int(cq[-1]) + 9, int(ck[-1]) + 5                 # rows past cu[B]: outside every sequence
    q = rnd((tq, H, D), dtype, 71).to(dev).requires_grad_(True)
    k = rnd((tk, Hk, D), dtype, 72).to(dev).requires_grad_(True)
    v = rnd((tk, Hk, D), dtype, 73).to(dev).requires_grad_(True)
    sentinel = torch.full((tq, H, D), 7.0, dtype=dtype, device=dev)
    with forced(lib, variant):
        o_pre, lse = ops.flash_attn_varlen_fwd(q.detach(), k.detach(), v.detach(), cq.to(dev), ck.to(dev), max(lq), max(lk), False, None,
                                               out=sentinel.clone(), window_size=window)
        out = tfa.flash_attn_varlen_func(q, k, v, cq.to(dev), ck.to(dev), max(lq), max(lk), window_size=window)
    dout = rnd((tq, H, D), dtype, 74).to(dev)
    out.backward(dout)
    torch.cuda.synchronize()
    assert bool((o_pre[int(cq[-1]):] == 7.0).all()), "rows outside every sequence must not be written"
    sc = 1.0 / math.sqrt(D)
    for b in range(len(lq)):
        q0, q1, k0, k1 = int(cq[b]), int(cq[b + 1]), int(ck[b]), int(ck[b + 1])
        if q1 == q0:
            continue
        qs = q.detach()[q0:q1].transpose(0, 1).unsqueeze(0)
        ks = k.detach()[k0:k1].transpose(0, 1).unsqueeze(0)
        vs = v.detach()[k0:k1].transpose(0, 1).unsqueeze(0)
        if k1 == k0:
            assert bool((out.detach()[q0:q1] == 0).all())
            continue
        ref, lref, _ = ref64(qs, ks, vs, *window, sc)
        assert (out.detach()[q0:q1].transpose(0, 1).unsqueeze(0).double().cpu() - ref).abs().max().item() <= 1e-2
        rg = ref_grads(qs, ks, vs, dout[q0:q1].transpose(0, 1).unsqueeze(0), *window, sc)
        for g, r, a, z in ((q.grad, rg[0], q0, q1), (k.grad, rg[1], k0, k1), (v.grad, rg[2], k0, k1)):
            gg = g[a:z].transpose(0, 1).unsqueeze(0).double().cpu()
            assert (gg - r).abs().max().item() <= 1e-2 * max(1.0, r.abs().max().item())
        dos = dout[q0:q1].transpose(0, 1).unsqueeze(0)
        form_ref.check_grads(None, tuple(g[a:z].transpose(0, 1).unsqueeze(0) for g, a, z in ((q.grad, q0, q1), (k.grad, k0, k1), (v.grad, k0, k1))), rg,
                             form_ref.bwd_bounds(qs, ks, vs, out.detach()[q0:q1].transpose(0, 1).unsqueeze(0), dos, sc, window=window), dtype, f"varlen seq {b}")
    for g, n in ((q.grad, int(cq[-1])), (k.grad, int(ck[-1])), (v.grad, int(ck[-1]))):
        assert bool((g[n:] == 0).all())


def test_varlen_window_graph_capture(lib, dev):
    from tiny_flash_attention_amd import ops

    dtype, H, D, window = torch.bfloat16, 2, 64, (80, 0)
    tq = 600
    q, k, v = (rnd((tq, H, D), dtype, s).to(dev) for s in (81, 82, 83))
    cq = torch.zeros(4, dtype=torch.int32, device=dev)
    ck = torch.zeros(4, dtype=torch.int32, device=dev)
    cq.copy_(cu_of([100, 200, 300]))
    ck.copy_(cu_of([100, 200, 300]))
    out = torch.zeros((tq, H, D), dtype=dtype, device=dev)
    ops.flash_attn_varlen_fwd(q, k, v, cq, ck, 300, 300, False, None, out=out, return_lse=False, window_size=window)   # warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.flash_attn_varlen_fwd(q, k, v, cq, ck, 300, 300, False, None, out=out, return_lse=False, window_size=window)
    cq.copy_(cu_of([250, 50, 300]))
    ck.copy_(cu_of([250, 50, 300]))
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    eager, _ = ops.flash_attn_varlen_fwd(q, k, v, cq, ck, 300, 300, False, None, window_size=window)
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
