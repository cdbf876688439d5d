"""GPU tests of apply_rotary_emb / apply_rotary_emb_qk_ (tfa_rotary) against an fp64 reference written here (tests/rotary_ref.py).

The bar, for every output element: |out - ref64| <= ulp_T(ref64) / 2 + 2^-21 * (|x1| + |x2|) — the one rounding to the output type plus a bound on the fp32
arithmetic (two products and a sum with |cos|, |sin| <= 1: 3 * 2^-24, doubled).  No measured tolerance.  Rows that must be unrotated are compared bit for bit."""
import pytest
import torch

import tiny_flash_attention_amd as tfa
from rotary_ref import excess, packed_positions, positions, rotary_ref64, tables, ulp_t

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, H, H2, RO = 2, 3, 1, 80
SHAPES = [(64, 64), (128, 32), (40, 16), (128, 128)]
DTYPES = [torch.float16, torch.bfloat16]


def bits(t):
    return t.contiguous().view(torch.int16).cpu()


def rand(shape, dtype, seed):
    return torch.empty(shape).normal_(0.0, 1.0, generator=torch.Generator().manual_seed(seed)).to(dtype)


def check(out, x, cos, sin, pos, interleaved, dtype, valid=None, conjugate=False):
    """out, x: (R, H, D) on the CPU.  Every element within the bar; unrotated rows bit for bit."""
    ref, mag, rotated = rotary_ref64(x, cos, sin, pos, interleaved, conjugate, valid)
    e = excess(out, ref, mag, dtype)
    assert e <= 0.0, f"an element exceeds ulp/2 + 2^-21 (|x1| + |x2|) by {e:.3e}"
    assert torch.equal(out[~rotated].view(torch.int16), x[~rotated].view(torch.int16)), "an unrotated row is not a bit-for-bit copy"
    return rotated


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,rd", SHAPES)
def test_values_offsets_and_inplace(D, rd, dtype, interleaved):
    """N = 1, 5, 70; tables of x's dtype and fp32; offsets as a host int, negative, past seqlen_ro, and as device tensors; in place = out of place in bits."""
    some_unrotated = False
    for N in (1, 5, 70):
        x = rand((B, N, H, D), dtype, seed=N + D)
        xd = x.to(DEV)
        for tdt in (dtype, torch.float32):
            cos, sin = tables(RO, rd, tdt)
            cd, sd = cos.to(DEV), sin.to(DEV)
            for off in (0, 7, -2, 20, [3, 75], [-1, 11]):
                arg = off if isinstance(off, int) else torch.tensor(off, dtype=torch.int32, device=DEV)
                out = tfa.apply_rotary_emb(xd, cd, sd, interleaved=interleaved, seqlen_offsets=arg)
                assert out.shape == xd.shape and out.dtype == dtype and out.data_ptr() != xd.data_ptr()
                rotated = check(out.cpu().reshape(B * N, H, D), x.reshape(B * N, H, D), cos, sin, positions(B, N, off), interleaved, dtype)
                some_unrotated |= not bool(rotated.all())
                xi = xd.clone()
                assert tfa.apply_rotary_emb(xi, cd, sd, interleaved=interleaved, inplace=True, seqlen_offsets=arg) is xi
                assert torch.equal(bits(xi), bits(out)), "in place differs from out of place"
        assert torch.equal(bits(xd), bits(x)), "the out-of-place call changed its input"
    assert some_unrotated


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_packed_form_padding_rows_and_a_strided_slice(dtype, interleaved):
    """Lengths [0, 1, 65, 7] plus 3 padding rows; x a slice of a packed (total, 3, H, D) projection; the binary search finds every row's sequence."""
    lens, pad = [0, 1, 65, 7], 3
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    total = cu[-1] + pad
    cud = torch.tensor(cu, dtype=torch.int32, device=DEV)
    for (D, rd), off in zip(SHAPES, (0, [5, 0, 10, 70], [5, 0, 20, 78], 9)):
        buf = rand((total, 3, H, D), dtype, seed=D + rd)
        bufd = buf.to(DEV)
        x, xd = buf[:, 1], bufd[:, 1]
        cos, sin = tables(RO, rd, torch.float32 if D == 128 else dtype)
        cd, sd = cos.to(DEV), sin.to(DEV)
        arg = off if isinstance(off, int) else torch.tensor(off, dtype=torch.int32, device=DEV)
        out = tfa.apply_rotary_emb(xd, cd, sd, interleaved=interleaved, seqlen_offsets=arg, cu_seqlens=cud, max_seqlen=max(lens))
        pos, valid = packed_positions(total, cu, off)
        rotated = check(out.cpu(), x, cos, sin, pos, interleaved, dtype, valid=valid)
        assert not rotated[-pad:].any() and rotated[:cu[-1]].sum() > 0
        tfa.apply_rotary_emb(xd, cd, sd, interleaved=interleaved, inplace=True, seqlen_offsets=arg, cu_seqlens=cud)
        assert torch.equal(bits(bufd[:, 1]), bits(out)), "in place differs from out of place"
        assert torch.equal(bits(bufd[:, 0]), bits(buf[:, 0])) and torch.equal(bits(bufd[:, 2]), bits(buf[:, 2])), "the neighbouring slices were touched"


@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_slice_of_a_batched_projection(dtype):
    N, D, rd = 5, 64, 64
    buf = rand((B, N, 3, H, D), dtype, seed=3)
    bufd = buf.to(DEV)
    cos, sin = tables(RO, rd, dtype)
    lens = torch.tensor([4, 60], dtype=torch.int32, device=DEV)
    out = tfa.apply_rotary_emb(bufd[:, :, 0], cos.to(DEV), sin.to(DEV), seqlen_offsets=lens)
    check(out.cpu().reshape(B * N, H, D), buf[:, :, 0].reshape(B * N, H, D), cos, sin, positions(B, N, [4, 60]), False, dtype)
    tfa.apply_rotary_emb(bufd[:, :, 0], cos.to(DEV), sin.to(DEV), seqlen_offsets=lens, inplace=True)
    assert torch.equal(bits(bufd[:, :, 0]), bits(out))
    assert torch.equal(bits(bufd[:, :, 1:]), bits(buf[:, :, 1:])), "k and v of the projection were touched"


def test_a_cu_seqlens_that_is_not_monotonic_rotates_only_rows_it_can_place():
    """Whatever cu_seqlens holds: a row comes back unrotated, or rotated as a row of a sequence b with cu[b] <= row < cu[b+1] — and nothing else is touched."""
    dtype, D, rd, total = torch.bfloat16, 64, 32, 14
    cu, off = [0, 9, 4, 6, 12], [1, 20, 40, 60]
    x = rand((total, H, D), dtype, seed=11)
    guard = rand((total + 8, H, D), dtype, seed=12).to(DEV)
    guard[4:4 + total] = x.to(DEV)
    cos, sin = tables(RO, rd, dtype)
    before = bits(guard)
    tfa.apply_rotary_emb(guard[4:4 + total], cos.to(DEV), sin.to(DEV), inplace=True, cu_seqlens=torch.tensor(cu, dtype=torch.int32, device=DEV),
                         seqlen_offsets=torch.tensor(off, dtype=torch.int32, device=DEV))
    after = bits(guard)
    assert torch.equal(after[:4], before[:4]) and torch.equal(after[4 + total:], before[4 + total:])
    out = guard[4:4 + total].cpu()
    for r in range(total):
        ok = torch.equal(out[r].view(torch.int16), x[r].view(torch.int16))
        for b in range(4):
            if not ok and cu[b] <= r < cu[b + 1]:
                ref, mag, _ = rotary_ref64(x[r:r + 1], cos, sin, torch.tensor([off[b] + r - cu[b]]), False)
                ok = excess(out[r:r + 1], ref, mag, dtype) <= 0.0
        assert ok, f"row {r} is neither a copy nor a rotation at a position cu_seqlens allows"


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_pair_call_equals_two_single_calls_in_bits(dtype, interleaved):
    for (D, rd), N in zip(SHAPES, (70, 5, 1, 70)):
        q, k = rand((B, N, H, D), dtype, seed=1).to(DEV), rand((B, N, H2, D), dtype, seed=2).to(DEV)
        cos, sin = (t.to(DEV) for t in tables(RO, rd, torch.float32 if D == 40 else dtype))
        lens = torch.tensor([6, 30], dtype=torch.int32, device=DEV)
        want_q = tfa.apply_rotary_emb(q, cos, sin, interleaved=interleaved, seqlen_offsets=lens)
        want_k = tfa.apply_rotary_emb(k, cos, sin, interleaved=interleaved, seqlen_offsets=lens)
        rq, rk = tfa.apply_rotary_emb_qk_(q, k, cos, sin, interleaved=interleaved, seqlen_offsets=lens)
        assert rq is q and rk is k
        assert torch.equal(bits(q), bits(want_q)) and torch.equal(bits(k), bits(want_k))
    # packed, q and k slices of one projection
    cu, total, D, rd = [0, 0, 1, 66, 73], 76, 64, 32
    qkv = rand((total, H + 2 * H2, D), dtype, seed=5).to(DEV)
    keep = qkv.clone()
    cud = torch.tensor(cu, dtype=torch.int32, device=DEV)
    lens = torch.tensor([0, 3, 9, 77], dtype=torch.int32, device=DEV)
    cos, sin = (t.to(DEV) for t in tables(RO, rd, dtype))
    want_q = tfa.apply_rotary_emb(qkv[:, :H], cos, sin, interleaved=interleaved, seqlen_offsets=lens, cu_seqlens=cud)
    want_k = tfa.apply_rotary_emb(qkv[:, H:H + H2], cos, sin, interleaved=interleaved, seqlen_offsets=lens, cu_seqlens=cud)
    tfa.apply_rotary_emb_qk_(qkv[:, :H], qkv[:, H:H + H2], cos, sin, interleaved=interleaved, seqlen_offsets=lens, cu_seqlens=cud)
    assert torch.equal(bits(qkv[:, :H]), bits(want_q)) and torch.equal(bits(qkv[:, H:H + H2]), bits(want_k))
    assert torch.equal(bits(qkv[:, H + H2:]), bits(keep[:, H + H2:])), "v of the projection was touched"


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_is_the_conjugate_rotation(dtype, interleaved):
    """torch.autograd.grad of (out * w).sum() against fp64 autograd of the reference: the same bar with dout = w in place of x; fixed-length and packed."""
    D, rd, N = 128, 32, 70
    cos, sin = tables(RO, rd, dtype)
    cd, sd = cos.to(DEV), sin.to(DEV)
    cu, total, off = [0, 0, 1, 66, 73], 76, [5, 0, 20, 78]
    for packed in (False, True):
        shape = (total, H, D) if packed else (B, N, H, D)
        x, w = rand(shape, dtype, seed=21), rand(shape, dtype, seed=22)
        xd = x.to(DEV).requires_grad_(True)
        if packed:
            kw = dict(cu_seqlens=torch.tensor(cu, dtype=torch.int32, device=DEV), seqlen_offsets=torch.tensor(off, dtype=torch.int32, device=DEV))
            pos, valid = packed_positions(total, cu, off)
        else:
            kw = dict(seqlen_offsets=15)
            pos, valid = positions(B, N, 15), None
        out = tfa.apply_rotary_emb(xd, cd, sd, interleaved=interleaved, **kw)
        (g,) = torch.autograd.grad((out * w.to(DEV)).sum(), xd)
        assert g.shape == xd.shape and g.dtype == dtype
        # fp64 autograd of the reference
        x64 = x.double().reshape(-1, H, D).requires_grad_(True)
        ro, half = cos.shape
        rot = (pos >= 0) & (pos < ro) if valid is None else (pos >= 0) & (pos < ro) & valid
        c = torch.where(rot[:, None], cos.double()[pos.clamp(0, ro - 1)], torch.ones(1, dtype=torch.float64))[:, None, :]
        s = torch.where(rot[:, None], sin.double()[pos.clamp(0, ro - 1)], torch.zeros(1, dtype=torch.float64))[:, None, :]
        x1, x2 = (x64[..., 0:rd:2], x64[..., 1:rd:2]) if interleaved else (x64[..., :half], x64[..., half:rd])
        o1, o2 = x1 * c - x2 * s, x1 * s + x2 * c
        rest = x64[..., rd:]
        loss = (torch.stack((o1, o2), -1).flatten(-2) if interleaved else torch.cat((o1, o2), -1))
        w64 = w.double().reshape(-1, H, D)
        (g64,) = torch.autograd.grad((loss * w64[..., :rd]).sum() + (rest * w64[..., rd:]).sum(), x64)
        ref, mag, _ = rotary_ref64(w.reshape(-1, H, D), cos, sin, pos, interleaved, conjugate=True, valid=valid)
        assert (ref - g64).abs().max().item() < 1e-12            # the conjugate rotation IS the gradient
        e = excess(g.cpu().reshape(-1, H, D), g64, mag, dtype)
        assert e <= 0.0, f"a gradient element exceeds the bar by {e:.3e}"
    # in place, on a non-leaf: the same gradient bits
    xd2 = x.to(DEV).requires_grad_(True)
    out2 = tfa.apply_rotary_emb(xd2 * 1, cd, sd, interleaved=interleaved, inplace=True, **kw)
    (g2,) = torch.autograd.grad((out2 * w.to(DEV)).sum(), xd2)
    assert torch.equal(bits(g2), bits(g))
    # the incoming gradient is read, never written; one in a layout the kernel does not take (no unit stride along D) is copied first: the same bits
    xd3 = x.to(DEV).requires_grad_(True)
    out3 = tfa.apply_rotary_emb(xd3, cd, sd, interleaved=interleaved, **kw)
    go = w.to(DEV)
    (g3,) = torch.autograd.grad(out3, xd3, grad_outputs=go, retain_graph=True)
    assert torch.equal(bits(go), bits(w)) and torch.equal(bits(g3), bits(g))
    go_t = go.transpose(-1, -2).contiguous().transpose(-1, -2)
    (g4,) = torch.autograd.grad(out3, xd3, grad_outputs=go_t)
    assert torch.equal(bits(g4), bits(g))


def test_rotation_then_conjugate_returns_x_within_two_roundings():
    """y = R x (rounded), z = R^T y (rounded; the backward run on y): |z - x| <= the first call's bar carried through R^T (|c|, |s| <= 1: the two errors of a
    pair add) + the second call's bar.  fp32 tables, so c^2 + s^2 = 1 to 2^-23 (a 2^-22 (|x1| + |x2|) term)."""
    D, rd, N = 64, 64, 70
    cos, sin = tables(RO, rd, torch.float32)
    cd, sd = cos.to(DEV), sin.to(DEV)
    for dtype in DTYPES:
        for interleaved in (False, True):
            x = rand((B, N, H, D), dtype, seed=31)
            xd = x.to(DEV).requires_grad_(True)
            y = tfa.apply_rotary_emb(xd, cd, sd, interleaved=interleaved, seqlen_offsets=3)
            (z,) = torch.autograd.grad(y, xd, grad_outputs=y.detach())
            pos = positions(B, N, 3)
            x3 = x.reshape(-1, H, D)
            yref, mag_x, _ = rotary_ref64(x3, cos, sin, pos, interleaved)
            e1 = 0.5 * ulp_t(yref, dtype) + 2.0 ** -21 * mag_x                      # the first call's bar, per element
            half = rd // 2
            pair = torch.zeros_like(e1)
            if interleaved:
                sm = e1[..., 0:rd:2] + e1[..., 1:rd:2]
                pair[..., 0:rd:2], pair[..., 1:rd:2] = sm, sm
            else:
                sm = e1[..., :half] + e1[..., half:rd]
                pair[..., :half], pair[..., half:rd] = sm, sm
            ycpu = y.detach().cpu().reshape(-1, H, D)
            zref, mag_y, _ = rotary_ref64(ycpu, cos, sin, pos, interleaved, conjugate=True)
            bar = pair + 2.0 ** -22 * mag_x + 0.5 * ulp_t(zref, dtype) + 2.0 ** -21 * mag_y
            d = (z.cpu().reshape(-1, H, D).double() - x3.double()).abs()
            assert (d - bar).max().item() <= 0.0
            assert torch.equal(bits(z)[..., rd:], bits(xd.detach())[..., rd:])
