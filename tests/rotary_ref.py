"""The fp64 reference of the rotary embedding and its error bar, shared by tests/test_rotary_gpu.py and tests/test_append_varlen_gpu.py (tests only)."""
import torch


def ulp_t(y, dtype):
    """Spacing of `dtype` (float16 / bfloat16) at |y| (fp64, elementwise), not less than its smallest subnormal."""
    mant, emin = (8, -126) if dtype == torch.bfloat16 else (11, -14)
    _, e = torch.frexp(y.abs().double())                     # |y| = m * 2^e, m in [0.5, 1): floor(log2 |y|) = e - 1
    return torch.exp2((e - 1).clamp_min(emin).double() - (mant - 1))


def positions(B, N, offsets):
    """(B * N,) positions of a (B, N, ...) tensor: offsets[b] + t (offsets: an int or a sequence of B ints)."""
    off = torch.as_tensor([offsets] * B if isinstance(offsets, int) else list(offsets), dtype=torch.long)
    return (off[:, None] + torch.arange(N)[None, :]).reshape(-1)


def packed_positions(total, cu, offsets):
    """(total,) positions of packed rows: offsets[b] + row - cu[b]; rows outside every sequence get None-like -1 with valid = False."""
    pos = torch.zeros(total, dtype=torch.long)
    valid = torch.zeros(total, dtype=torch.bool)
    for b in range(len(cu) - 1):
        for r in range(cu[b], min(cu[b + 1], total)):
            pos[r] = (offsets if isinstance(offsets, int) else offsets[b]) + r - cu[b]
            valid[r] = True
    return pos, valid


def rotary_ref64(x, cos, sin, pos, interleaved, conjugate=False, valid=None):
    """x (R, H, D) of any float dtype, cos / sin (seqlen_ro, rotary_dim / 2) as stored, pos (R,) long.  Returns (ref, mag, rotated): the exact (fp64) result, the
    |x1| + |x2| of every element's pair (0 for copied elements) and the (R,) mask of the rows that are rotated (the others must come back bit for bit)."""
    x = x.double()
    ro, half = cos.shape
    rd = 2 * half
    rotated = (pos >= 0) & (pos < ro)
    if valid is not None:
        rotated &= valid
    idx = pos.clamp(0, ro - 1)
    c = cos.double()[idx][:, None, :]
    s = sin.double()[idx][:, None, :]
    if conjugate:
        s = -s
    if interleaved:
        x1, x2 = x[..., 0:rd:2], x[..., 1:rd:2]
    else:
        x1, x2 = x[..., :half], x[..., half:rd]
    o1, o2 = x1 * c - x2 * s, x1 * s + x2 * c
    m = x1.abs() + x2.abs()
    ref, mag = x.clone(), torch.zeros_like(x)
    if interleaved:
        ref[..., 0:rd:2], ref[..., 1:rd:2] = o1, o2
        mag[..., 0:rd:2], mag[..., 1:rd:2] = m, m
    else:
        ref[..., :half], ref[..., half:rd] = o1, o2
        mag[..., :half], mag[..., half:rd] = m, m
    keep = ~rotated
    ref[keep] = x[keep]
    mag[keep] = 0.0
    return ref, mag, rotated


def excess(out, ref, mag, dtype):
    """max over elements of |out - ref| - (ulp_T(ref) / 2 + 2^-21 * mag): <= 0 when every element meets the bar (one rounding + the fp32 arithmetic)."""
    return ((out.double() - ref).abs() - (0.5 * ulp_t(ref, dtype) + 2.0 ** -21 * mag)).max().item()


def tables(ro, rd, dtype, base=10000.0):
    """cos / sin (ro, rd / 2) of the usual frequencies, rounded to `dtype`."""
    inv = 1.0 / (base ** (torch.arange(0, rd, 2, dtype=torch.float64) / rd))
    ang = torch.arange(ro, dtype=torch.float64)[:, None] * inv[None, :]
    return ang.cos().to(dtype), ang.sin().to(dtype)
