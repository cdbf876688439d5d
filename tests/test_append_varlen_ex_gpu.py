"""GPU tests of ``kvcache_append_varlen`` with its three keywords (tfa_kvcache_append_varlen_ex): e4m3 caches with ``k_descale`` / ``v_descale`` and ``q=``
rotated in place in the append's launch.

Every pool and q comparison is BIT FOR BIT (torch.equal on integer views of the whole tensor): the expected e4m3 bytes are built on the CPU with
``(x.float() / d).clamp(-448, 448).to(torch.float8_e4m3fn)`` — the conversion tests/test_kvcache_fp8_gpu.py relies on as the kernel's rule — into a pool
pre-filled with a sentinel byte pattern that includes NaN codes, so a stray store anywhere shows up; the expected q is what ``apply_rotary_emb(..., inplace=True)``
leaves on a clone.  One exception to bytes: where the input is NaN the stored byte must be a NaN code, either of e4m3fn's two (0x7f / 0xff) — the sign of the
NaN an fp32 division returns is the device's own, and tfa_kvcache_append_fp8's bytes, which this append shares, carry it.
End to end (the bars of this kernel family, include/tfa.h: 16-bit out |d| <= 1e-2, LSE |d| <= 1e-4 * max(1, |ref|), +inf exactly on rows that see no key; q std
1.0, K / V std 0.5): append + ``flash_attn_with_kvcache(cu_seqlens_q=)`` over a paged fp8 pool against fp64 attention over the CPU-built decoded pool and the
CPU-rotated q.  H8 Hk2 unless said otherwise."""
import math

import pytest
import torch

import tiny_flash_attention_amd as tfa
from rotary_ref import rotary_ref64, tables

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OUT_BAR, LSE_BAR = 1e-2, 1e-4
E4M3 = torch.float8_e4m3fn
H, HK = 8, 2
NEW = [1, 0, 7, 70, 3]                   # a sequence without rows; the 70 spans two 64-key pages
CACHED = [63, 5, 60, 120, 0]             # rows on both sides of a page boundary (63 | 64; 60 .. 66)
B = len(NEW)
PAD = 3                                  # packed rows behind cu[B]: dropped
DTYPES = [torch.bfloat16, torch.float16]


def cumsum0(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return cu


def randn(gen, *shape, dtype, std=0.5):
    return (torch.randn(*shape, generator=gen, dtype=torch.float32) * std).to(dtype)


def descales(gen, lo=0.006, hi=0.012, b=B):
    """Distinct per-(b, hk) descales, none a power of two; std-0.5 rows / these use the e4m3 range without reaching the clamp."""
    d = lo + (hi - lo) * torch.rand(b, HK, generator=gen, dtype=torch.float32)
    assert d.unique().numel() == d.numel() and not (torch.frexp(d)[0] == 0.5).any()
    return d


def sentinel8(shape, shift=0):
    """An e4m3 pool full of a byte pattern no append produces by accident; every fifth byte is the NaN code."""
    n = math.prod(shape)
    b = ((torch.arange(n, dtype=torch.int64) * 149 + 77 + shift) % 256).to(torch.uint8)
    b[::5] = 0x7F
    return b.view(shape).view(E4M3)


def sentinel16(shape, dtype):
    n = math.prod(shape)
    b = ((torch.arange(n, dtype=torch.int64) * 40503 + 12345) % 65536 - 32768).to(torch.int16)
    b[::5] = 0x7FFF
    return b.view(shape).view(dtype)


def raw(t):
    return t.contiguous().view(torch.uint8 if t.element_size() == 1 else torch.int16).cpu()


def quantise(rows, d):
    """The append's rule on the CPU: rows (n, HK, D) of any float dtype, d (HK,) float32 -> e4m3."""
    return (rows.float() / d.view(1, HK, 1)).clamp(-448.0, 448.0).to(E4M3)


def packed_qkv(gen, total, D, dtype, heads=H):
    """One packed projection (total, heads + 2 HK, D): q = [:, :heads], k = [:, heads:heads + HK], v = [:, heads + HK:]; q std 1.0, k / v std 0.5."""
    qkv = randn(gen, total, heads + 2 * HK, D, dtype=dtype)
    qkv[:, :heads] = randn(gen, total, heads, D, dtype=dtype, std=1.0)
    return qkv


def split(qkv, heads=H):
    return qkv[:, :heads], qkv[:, heads:heads + HK], qkv[:, heads + HK:]


def shuffled_table(gen, mb, spare=3, b=B):
    nb = b * mb + spare
    return nb, torch.randperm(nb, generator=gen)[: b * mb].view(b, mb).to(torch.int32)


def expected_pool(pool, rows, d, cu, cached, bt, page, cap):
    """The CPU mirror of the append into a (num_pages, page, HK, D) pool — or, bt None, a (B, cap, HK, D) cache: drops as the header states them.  d (B, HK): the
    pool is e4m3 and the rows are quantised with their SEQUENCE's descales; d None: a 16-bit pool, rows copied."""
    want = pool.clone()
    w = want.view(torch.uint8) if d is not None else want
    for b in range(len(cached)):
        n = cu[b + 1] - cu[b]
        if n <= 0:
            continue
        src = rows[cu[b]:cu[b + 1]]
        src = quantise(src, d[b]).view(torch.uint8) if d is not None else src
        for t in range(n):
            pos = cached[b] + t
            if pos < 0 or pos >= cap:
                continue
            if bt is None:
                w[b, pos] = src[t]
                continue
            pg = int(bt[b, pos // page])
            if 0 <= pg < pool.shape[0]:
                w[pg, pos % page] = src[t]
    return want


def rows_written(want, before):
    return (raw(want) != raw(before)).any(-1).any(-1).sum().item()


def i32(a):
    return torch.tensor(a, dtype=torch.int32, device=DEV)


def dev(t):
    return None if t is None else t.to(DEV)


def append(k, v, kp, vp, cu, cached, bt, **kw):
    assert tfa.kvcache_append_varlen(k, v, kp, vp, i32(cu), i32(cached), dev(bt), **kw) is None
    torch.cuda.synchronize()


# ---- 1. fp8 pool bytes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [16, 64, 128])
@pytest.mark.parametrize("page", [64, 256])
def test_fp8_pool_bytes(page, D, dtype):
    gen = torch.Generator().manual_seed(page + D)
    cu = cumsum0(NEW)
    total = cu[-1] + PAD
    qkv = packed_qkv(gen, total, D, dtype)
    _, k, v = split(qkv)
    kd, vd = descales(gen), descales(gen)
    mb = 256 // page
    nb, bt = shuffled_table(gen, mb)
    kp0, vp0 = sentinel8((nb, page, HK, D)), sentinel8((nb, page, HK, D), shift=31)
    want_k = expected_pool(kp0, k, kd, cu, CACHED, bt, page, mb * page)
    want_v = expected_pool(vp0, v, vd, cu, CACHED, bt, page, mb * page)
    qkv_d, kp, vp = qkv.to(DEV), kp0.to(DEV), vp0.to(DEV)
    _, k_d, v_d = split(qkv_d)
    append(k_d, v_d, kp, vp, cu, CACHED, bt, k_descale=kd.to(DEV), v_descale=vd.to(DEV))
    assert torch.equal(raw(kp), raw(want_k)), "k pool differs from the pool built on the CPU"
    assert torch.equal(raw(vp), raw(want_v)), "v pool differs from the pool built on the CPU"
    assert torch.equal(raw(qkv_d), raw(qkv)), "the new rows were modified"
    assert rows_written(want_k, kp0) == sum(NEW)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fp8_contiguous_cache_with_an_expanded_unit_scale_and_a_strided_descale(dtype):
    gen = torch.Generator().manual_seed(3)
    D, cap, cu = 64, 256, cumsum0(NEW)
    total = cu[-1] + PAD
    qkv = packed_qkv(gen, total, D, dtype)
    _, k, v = split(qkv)
    vd_wide = torch.stack([descales(gen), descales(gen)], dim=-1)                  # (B, HK, 2): v_descale = [..., 0], strides (2 HK, 2)
    kc0, vc0 = sentinel8((B, 2 * cap, HK, D))[:, :cap], sentinel8((B, cap, HK, D), shift=9)       # k: a strided view, sequences 2 * cap rows apart
    want_k = expected_pool(kc0, k, torch.ones(B, HK), cu, CACHED, None, 0, cap)
    want_v = expected_pool(vc0, v, vd_wide[..., 0], cu, CACHED, None, 0, cap)
    whole = sentinel8((B, 2 * cap, HK, D)).to(DEV)
    kc, vc, qkv_d = whole[:, :cap], vc0.to(DEV), qkv.to(DEV)
    _, k_d, v_d = split(qkv_d)
    append(k_d, v_d, kc, vc, cu, CACHED, None, k_descale=torch.ones(1, 1, device=DEV).expand(B, HK), v_descale=vd_wide.to(DEV)[..., 0])
    assert torch.equal(raw(kc), raw(want_k)) and torch.equal(raw(vc), raw(want_v))
    assert torch.equal(raw(whole[:, cap:]), raw(sentinel8((B, 2 * cap, HK, D))[:, cap:])), "rows behind the capacity were written"


# ---- 2. special values --------------------------------------------------------------------------------------------------------------------------
def special_rows(dtype, d, D):
    """tests/test_kvcache_fp8_gpu.py's: rows whose quotients x / d hit the clamp, the ties and the subnormal range of e4m3 (d: this row's descale, a float)."""
    targets = [448.0, 449.0, 464.0, 465.0, 480.0, 1000.0, 1e6, -448.0, -464.0, -1e5, 0.0, -0.0, 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, 5 * 2.0 ** -10, 2.0 ** -11,
               0.0146, 0.0156, 2.0 ** -6, 1.0625, 1.1875, 1.3125, 17.0, 18.0, 19.0, 22.0, 26.0, 208.0, 240.0, 432.0, 447.0, float("inf"), float("-inf")]
    x = torch.tensor(targets, dtype=torch.float32) * d
    return torch.cat([x, x.flip(0)])[:D].to(dtype) if 2 * len(targets) >= D else torch.cat([x] * (D // len(targets) + 1))[:D].to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fp8_clamp_ties_subnormals_and_nan(dtype):
    gen = torch.Generator().manual_seed(11)
    D, page, mb, cu = 64, 64, 4, cumsum0(NEW)
    total = cu[-1] + PAD
    qkv = packed_qkv(gen, total, D, dtype)
    _, k, v = split(qkv)
    kd, vd = descales(gen), descales(gen)
    for b in range(B):
        for t in range(min(NEW[b], 2)):                                            # the first rows of every sequence: K head 0, V head 1
            k[cu[b] + t, 0] = special_rows(dtype, float(kd[b, 0]), D)
            v[cu[b] + t, 1] = special_rows(dtype, float(vd[b, 1]), D)
    k[cu[3] + 5, 1, 5] = float("nan")                                              # a NaN input stays NaN
    kq = quantise(k[cu[3]:cu[4]], kd[3]).float()
    assert (kq.abs() == 448).any() and ((kq != 0) & (kq.abs() < 2.0 ** -6)).any() and torch.isnan(kq).sum() == 1    # the inputs reach the clamp and the subnormals
    nb, bt = shuffled_table(gen, mb)
    kp0, vp0 = torch.zeros(nb, page, HK, D, dtype=torch.uint8).view(E4M3), torch.zeros(nb, page, HK, D, dtype=torch.uint8).view(E4M3)
    want_k = expected_pool(kp0, k, kd, cu, CACHED, bt, page, mb * page)
    want_v = expected_pool(vp0, v, vd, cu, CACHED, bt, page, mb * page)
    assert torch.isnan(want_k.float()).sum() == 1 and not torch.isnan(want_v.float()).any()
    qkv_d, kp, vp = qkv.to(DEV), kp0.to(DEV), vp0.to(DEV)
    _, k_d, v_d = split(qkv_d)
    append(k_d, v_d, kp, vp, cu, CACHED, bt, k_descale=kd.to(DEV), v_descale=vd.to(DEV))
    for got, want, name in ((kp, want_k, "k"), (vp, want_v, "v")):
        g, w = raw(got), raw(want)
        nan = (w & 0x7F) == 0x7F                                                   # e4m3fn has two NaN codes, 0x7f and 0xff: "NaN stays NaN" fixes no sign (the
        assert torch.equal((g & 0x7F) == 0x7F, nan), f"{name} pool: NaN elsewhere than expected"      # fp32 division's NaN carries the device's, not the CPU's)
        bad = (g != w) & ~nan
        assert not bad.any(), f"{name} pool: {int(bad.sum())} bytes differ, e.g. got {g[bad][:6].tolist()} want {w[bad][:6].tolist()}"


# ---- 3. equal counts: the bytes of flash_attn_with_kvcache(k=, v=) ------------------------------------------------------------------------------
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fp8_equal_counts_leave_the_bytes_of_flash_attn_with_kvcache(dtype, paged):
    gen = torch.Generator().manual_seed(4)
    n_new, D, page, cap = 3, 64, 64, 256
    lens0 = [0, 63, 64, 130, 254]                                                  # the last sequence loses its third row to the capacity in both calls
    kn, vn = randn(gen, B, n_new, HK, D, dtype=dtype).to(DEV), randn(gen, B, n_new, HK, D, dtype=dtype).to(DEV)
    q = randn(gen, B, n_new, H, D, dtype=dtype, std=1.0).to(DEV)
    kd, vd = descales(gen).to(DEV), descales(gen).to(DEV)
    lens = i32(lens0)
    if paged:
        nb, bt = shuffled_table(gen, cap // page)
        shape, bt = (nb, page, HK, D), bt.to(DEV)
    else:
        shape, bt = (B, cap, HK, D), None
    pools = [[sentinel8(shape).to(DEV), sentinel8(shape, shift=5).to(DEV)] for _ in range(2)]
    for p in pools[0] + pools[1]:                                                  # (the attention reads the pool: finite codes instead of the NaN ones)
        p.view(torch.uint8)[p.view(torch.uint8) == 0x7F] = 0x38
    before = raw(pools[1][0])
    tfa.flash_attn_with_kvcache(q, pools[0][0], pools[0][1], kn, vn, cache_seqlens=lens, block_table=bt, causal=True, num_splits=1, k_descale=kd, v_descale=vd)
    cu = torch.arange(B + 1, dtype=torch.int32, device=DEV) * n_new
    tfa.kvcache_append_varlen(kn.view(B * n_new, HK, D), vn.view(B * n_new, HK, D), pools[1][0], pools[1][1], cu, lens, bt, k_descale=kd, v_descale=vd)
    torch.cuda.synchronize()
    assert torch.equal(raw(pools[0][0]), raw(pools[1][0])) and torch.equal(raw(pools[0][1]), raw(pools[1][1]))
    assert (raw(pools[1][0]) != before).any(-1).any(-1).sum().item() == B * n_new - 1


# ---- 4. drops -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_fp8_capacity_negative_lengths_and_bad_table_entries_drop_their_rows_and_nothing_else(dtype):
    """Paged, capacity 3 x 64 = 192: sequence 3 (130 cached + 70 new) loses its rows at positions >= 192; sequence 4 starts at -2 and loses two rows; a table
    entry of -1 and one of num_pages drop the rows that map to them."""
    gen = torch.Generator().manual_seed(9)
    page, mb, D, cu = 64, 3, 64, cumsum0(NEW)
    cached = [63, 5, 60, 130, -2]
    total = cu[-1] + PAD
    qkv = packed_qkv(gen, total, D, dtype)
    _, k, v = split(qkv)
    kd, vd = descales(gen), descales(gen)
    nb, bt = shuffled_table(gen, mb)
    for bad in (None, (2, 1, -1), (3, 2, nb)):                                    # sequence 2 appends into blocks 0 and 1 (60 .. 63 | 64 .. 66), sequence 3 into block 2 (130 .. 191)
        table = bt.clone()
        if bad:
            table[bad[0], bad[1]] = bad[2]
        kp0, vp0 = sentinel8((nb, page, HK, D)), sentinel8((nb, page, HK, D), shift=7)
        want_k = expected_pool(kp0, k, kd, cu, cached, table, page, mb * page)
        want_v = expected_pool(vp0, v, vd, cu, cached, table, page, mb * page)
        kp, vp, qkv_d = kp0.to(DEV), vp0.to(DEV), qkv.to(DEV)
        _, k_d, v_d = split(qkv_d)
        append(k_d, v_d, kp, vp, cu, cached, table, k_descale=kd.to(DEV), v_descale=vd.to(DEV))
        assert torch.equal(raw(kp), raw(want_k)) and torch.equal(raw(vp), raw(want_v)), f"bad entry {bad}"
        assert rows_written(want_k, kp0) == {None: 1 + 7 + 62 + 1, (2, 1, -1): 1 + 4 + 62 + 1, (3, 2, nb): 1 + 7 + 1}[bad]


# ---- 5. fused rotary into an fp8 pool -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fp8_fused_rotary_equals_rotating_first_and_appending_plain(dtype, interleaved):
    """The pool holds the bytes apply_rotary_emb(k, cu_seqlens=cu, seqlen_offsets=cache_seqlens) + the plain fp8 append leave; V is only quantised; positions at
    and behind seqlen_ro (180: sequence 3 reaches 189) are stored unrotated."""
    gen = torch.Generator().manual_seed(5)
    page, mb, ro, cu = 64, 4, 180, cumsum0(NEW)
    total = cu[-1] + PAD
    for D, rd, tdt in ((64, 32, dtype), (64, 64, torch.float32), (128, 128, dtype), (64, 32, torch.float32), (16, 16, dtype)):
        qkv = packed_qkv(gen, total, D, dtype)
        _, _, v = split(qkv)
        qkv_d = qkv.to(DEV)
        _, k_d, v_d = split(qkv_d)
        kd, vd = descales(gen), descales(gen)
        nb, bt = shuffled_table(gen, mb)
        cos, sin = (t.to(DEV) for t in tables(ro, rd, tdt))
        pools = [[sentinel8((nb, page, HK, D)).to(DEV), sentinel8((nb, page, HK, D), shift=1).to(DEV)] for _ in range(2)]
        cud, lens, btd, kdd, vdd = i32(cu), i32(CACHED), bt.to(DEV), kd.to(DEV), vd.to(DEV)
        k_rot = tfa.apply_rotary_emb(k_d, cos, sin, interleaved=interleaved, cu_seqlens=cud, seqlen_offsets=lens)
        tfa.kvcache_append_varlen(k_rot, v_d, pools[0][0], pools[0][1], cud, lens, btd, k_descale=kdd, v_descale=vdd)
        tfa.kvcache_append_varlen(k_d, v_d, pools[1][0], pools[1][1], cud, lens, btd, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=interleaved,
                                  k_descale=kdd, v_descale=vdd)
        torch.cuda.synchronize()
        assert torch.equal(raw(pools[0][0]), raw(pools[1][0])), f"fused rotary differs from rotate-then-append (D {D}, rotary_dim {rd}, tables {tdt})"
        assert torch.equal(raw(pools[0][1]), raw(pools[1][1]))
        assert not torch.equal(raw(k_rot), raw(k_d)) and torch.equal(raw(qkv_d), raw(qkv))
        want_k = expected_pool(sentinel8((nb, page, HK, D)), k_rot.cpu(), kd, cu, CACHED, bt, page, mb * page)       # ... and both are the CPU's bytes of the rotated rows
        want_v = expected_pool(sentinel8((nb, page, HK, D), shift=1), v, vd, cu, CACHED, bt, page, mb * page)
        assert torch.equal(raw(pools[1][0]), raw(want_k)) and torch.equal(raw(pools[1][1]), raw(want_v))


# ---- 6. q= ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [8, 2])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_q_is_rotated_in_place_in_the_appends_launch(dtype, interleaved, fp8, heads):
    """q = qkv[:, :heads] of a packed (total, heads + 2 HK, D) projection whose other slices are k and v; rotary_dim 32 < D 64.  Sequence 4 sits at the capacity
    (256): its K rows are dropped, its q rows are rotated — but for its last one, whose position 258 is the first one behind the tables."""
    gen = torch.Generator().manual_seed(6 + heads)
    D, rd, page, mb, ro, cu = 64, 32, 64, 4, 258, cumsum0(NEW)
    cached = [63, 5, 60, 120, 256]
    total = cu[-1] + PAD
    qkv = packed_qkv(gen, total, D, dtype, heads)
    nb, bt = shuffled_table(gen, mb)
    cos, sin = (t.to(DEV) for t in tables(ro, rd, torch.float32 if interleaved else dtype))
    cud, lens, btd = i32(cu), i32(cached), bt.to(DEV)
    kw = dict(rotary_cos=cos, rotary_sin=sin, rotary_interleaved=interleaved)
    if fp8:
        kw.update(k_descale=descales(gen).to(DEV), v_descale=descales(gen).to(DEV))
        fresh = lambda: [sentinel8((nb, page, HK, D)).to(DEV), sentinel8((nb, page, HK, D), shift=1).to(DEV)]
    else:
        fresh = lambda: [sentinel16((nb, page, HK, D), dtype).to(DEV), sentinel16((nb, page, HK, D), dtype).roll(1, 0).to(DEV)]
    # the two launches of the parent commit on one copy ...
    ref_qkv, ref_pools = qkv.to(DEV), fresh()
    rq, rk, rv = split(ref_qkv, heads)
    tfa.kvcache_append_varlen(rk, rv, ref_pools[0], ref_pools[1], cud, lens, btd, **kw)
    assert tfa.apply_rotary_emb(rq, cos, sin, interleaved=interleaved, inplace=True, seqlen_offsets=lens, cu_seqlens=cud) is rq
    # ... and the one launch on another
    got_qkv, pools = qkv.to(DEV), fresh()
    gq, gk, gv = split(got_qkv, heads)
    tfa.kvcache_append_varlen(gk, gv, pools[0], pools[1], cud, lens, btd, q=gq, **kw)
    torch.cuda.synchronize()
    assert torch.equal(raw(got_qkv), raw(ref_qkv)), "q differs from apply_rotary_emb(..., inplace=True), or bytes of the projection outside q changed"
    assert torch.equal(raw(pools[0]), raw(ref_pools[0])) and torch.equal(raw(pools[1]), raw(ref_pools[1])), "the pool differs from the same call without q"
    got, orig = raw(got_qkv), raw(qkv)
    assert torch.equal(got[:, heads:], orig[:, heads:]), "k / v were modified"
    assert torch.equal(got[:, :heads, rd:], orig[:, :heads, rd:]), "elements behind rotary_dim were modified"
    assert torch.equal(got[cu[-1]:], orig[cu[-1]:]), "a row outside every sequence was modified"
    changed = (got[:, :heads] != orig[:, :heads]).any(-1).any(-1)
    assert changed[:cu[-1] - 1].all() and not changed[cu[-1] - 1], "every row with a table position is rotated; position 258 has none"
    assert (raw(pools[0]) != raw(fresh()[0])).any(-1).any(-1).sum().item() == 1 + 7 + 70, "sequence 4's K rows are beyond the capacity: dropped"


# ---- 7. end to end --------------------------------------------------------------------------------------------------------------------------------
def rows_of(cu, total_q, max_q):
    """(q0_b, nq_b) as every work item of the attention clamps them (include/tfa.h)."""
    res = []
    for b in range(len(cu) - 1):
        q0 = min(max(int(cu[b]), 0), total_q)
        res.append((q0, min(max(int(cu[b + 1]) - int(cu[b]), 0), min(max_q, total_q - q0))))
    return res


def reference(q, k_pool, v_pool, cu, lens, bt, scale, max_q, kd, vd):
    """tests/test_kvcache_varlenq_gpu.py's: fp64 causal attention of every sequence's rows over its own decoded, descaled keys of a paged pool: out (total_q, H, D),
    lse (H, total_q); rows that see no key: out = 0, lse = +inf."""
    q, k_pool, v_pool = q.double(), k_pool.double(), v_pool.double()
    total_q, Hq, D = q.shape
    G, page = Hq // HK, k_pool.shape[1]
    cap = page * bt.shape[1]
    out = torch.zeros(total_q, Hq, D, dtype=torch.float64)
    lse = torch.full((Hq, total_q), math.inf, dtype=torch.float64)
    for b, (q0, nq) in enumerate(rows_of(cu, total_q, max_q)):
        n = min(max(int(lens[b]), 0), cap)
        if n == 0 or nq == 0:
            continue
        gather = lambda pool: torch.cat([pool[int(bt[b, i])] for i in range((n + page - 1) // page)], 0)[:n]
        k = (gather(k_pool) * kd[b].double().view(1, HK, 1)).repeat_interleave(G, dim=1)
        v = (gather(v_pool) * vd[b].double().view(1, HK, 1)).repeat_interleave(G, dim=1)
        s = torch.einsum("qhd,khd->hqk", q[q0:q0 + nq], k) * scale
        i, j = torch.arange(nq).view(nq, 1), torch.arange(n).view(1, n)
        s = s.masked_fill(j > i + (n - nq), -math.inf)
        l = torch.logsumexp(s, dim=-1)
        seen = torch.isfinite(l)
        p = torch.exp(s - torch.where(seen, l, torch.zeros_like(l)).unsqueeze(-1))
        p = torch.where(seen.unsqueeze(-1), p, torch.zeros_like(p))
        out[q0:q0 + nq] = torch.einsum("hqk,khd->qhd", p, v)
        lse[:, q0:q0 + nq] = torch.where(seen, l, torch.full_like(l, math.inf))
    return out, lse


def assert_matches(out, lse, ref_out, ref_lse, what):
    out, lse = out.double().cpu(), lse.double().cpu()
    assert out.shape == ref_out.shape and lse.shape == ref_lse.shape
    assert not torch.isnan(out).any() and not torch.isnan(lse).any(), f"{what}: NaN in the result"
    err = (out - ref_out).abs().max().item()
    inf_ref = torch.isinf(ref_lse)
    assert torch.equal(torch.isinf(lse) & (lse > 0), inf_ref), f"{what}: lse = +inf on other rows than the reference"
    fin = ~inf_ref
    rel = ((lse[fin] - ref_lse[fin]).abs() / ref_lse[fin].abs().clamp(min=1.0)).max().item()
    print(f"{what}: max|d out| = {err:.3e} (bar {OUT_BAR}), max LSE err = {rel:.3e} (bar {LSE_BAR}), empty rows = {int(inf_ref.sum())}")
    assert err <= OUT_BAR, f"{what}: max|d out| = {err}"
    assert rel <= LSE_BAR, f"{what}: LSE error {rel}"
    if inf_ref.any():
        assert (out.transpose(0, 1)[inf_ref] == 0).all(), f"{what}: out != 0 on rows that see no key"


E2E_NQ = [1, 1, 40, 1, 5]                # decode rows, one chunk of 40 rows (G = 4: 160 packed rows, two query blocks), and a sequence that starts at -2:
E2E_CACHED = [300, 63, 89, 0, -2]        # its first two K rows are dropped, its first two q rows see no key (lse = +inf) and are not rotated


def e2e_pool(gen, dtype, D, page, mb, kd, vd):
    """A paged e4m3 pool that holds the cached keys of E2E_CACHED (std 0.5, quantised on the CPU), NaN codes everywhere else."""
    nb, bt = shuffled_table(gen, mb)
    kp = torch.full((nb, page, HK, D), 0x7F, dtype=torch.uint8).view(E4M3)
    vp = torch.full((nb, page, HK, D), 0x7F, dtype=torch.uint8).view(E4M3)
    for b, c in enumerate(E2E_CACHED):
        if c <= 0:
            continue
        kq, vq = quantise(randn(gen, c, HK, D, dtype=dtype), kd[b]), quantise(randn(gen, c, HK, D, dtype=dtype), vd[b])
        for pos in range(c):
            kp.view(torch.uint8)[int(bt[b, pos // page]), pos % page] = kq.view(torch.uint8)[pos]
            vp.view(torch.uint8)[int(bt[b, pos // page]), pos % page] = vq.view(torch.uint8)[pos]
    return kp, vp, bt


def cpu_step(qkv, kp, vp, bt, cu, cached, cos, sin, interleaved, kd, vd, page, mb):
    """The step on the CPU: (the rotated q, the pools after the append) — rotary in fp64 rounded once to the 16-bit type, then the append's quantisation."""
    dtype, total = qkv.dtype, qkv.shape[0]
    q, k, v = split(qkv)
    pos = torch.zeros(total, dtype=torch.long)
    for b in range(len(cached)):
        pos[cu[b]:cu[b + 1]] = cached[b] + torch.arange(cu[b + 1] - cu[b])
    q_rot = rotary_ref64(q, cos, sin, pos, interleaved)[0].to(dtype)
    k_rot = rotary_ref64(k, cos, sin, pos, interleaved)[0].to(dtype)
    return q_rot, expected_pool(kp, k_rot, kd, cu, cached, bt, page, mb * page), expected_pool(vp, v, vd, cu, cached, bt, page, mb * page)


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_unified_batch_over_an_fp8_pool_append_with_q_then_attention(dtype, interleaved):
    gen = torch.Generator().manual_seed(7)
    D, rd, page, mb, ro = 64, 32, 64, 8, 512
    cu = cumsum0(E2E_NQ)
    total = cu[-1]
    kd, vd = descales(gen), descales(gen)
    kp, vp, bt = e2e_pool(gen, dtype, D, page, mb, kd, vd)
    qkv = packed_qkv(gen, total, D, dtype)
    cos, sin = tables(ro, rd, torch.float32)
    q_rot, want_k, want_v = cpu_step(qkv, kp, vp, bt, cu, E2E_CACHED, cos, sin, interleaved, kd, vd, page, mb)
    assert want_k.float().abs().nan_to_num(0).max() < 448 and want_v.float().abs().nan_to_num(0).max() < 448
    lens_now = [c + n for c, n in zip(E2E_CACHED, E2E_NQ)]
    scale = 1.0 / math.sqrt(D)
    ref_out, ref_lse = reference(q_rot, want_k.float(), want_v.float(), cu, lens_now, bt, scale, max(E2E_NQ), kd, vd)
    assert int(torch.isinf(ref_lse).sum()) == 2 * H
    qkv_d, kp_d, vp_d, btd, kdd, vdd = qkv.to(DEV), kp.to(DEV), vp.to(DEV), bt.to(DEV), kd.to(DEV), vd.to(DEV)
    q_d, k_d, v_d = split(qkv_d)
    cud, lens = i32(cu), i32(E2E_CACHED)
    tfa.kvcache_append_varlen(k_d, v_d, kp_d, vp_d, cud, lens, btd, rotary_cos=cos.to(DEV), rotary_sin=sin.to(DEV), rotary_interleaved=interleaved, q=q_d,
                              k_descale=kdd, v_descale=vdd)
    lens_d = lens + torch.diff(cud)
    assert lens_d.tolist() == lens_now
    out, lse = tfa.flash_attn_with_kvcache(q_d, kp_d, vp_d, cache_seqlens=lens_d, block_table=btd, causal=True, cu_seqlens_q=cud, max_seqlen_q=max(E2E_NQ),
                                           k_descale=kdd, v_descale=vdd, return_softmax_lse=True)
    torch.cuda.synchronize()
    assert_matches(out, lse, ref_out, ref_lse, f"fp8 unified batch {dtype} interleaved={interleaved}")
    assert torch.equal(raw(vp_d), raw(want_v)), "the V pool is the CPU's, byte for byte (K's rotation is fp32 on the device, fp64 here)"


# ---- 8. graph capture -----------------------------------------------------------------------------------------------------------------------------
def test_captured_two_call_step_replays_at_advanced_lengths():
    """append(q=, descales) + flash_attn_with_kvcache(cu_seqlens_q=), captured once on one stream after a warm-up, replayed once after q / k / v were overwritten and
    cache_seqlens advanced in place: pool bytes and out equal the eager step at the advanced lengths."""
    gen = torch.Generator().manual_seed(8)
    dtype, D, rd, page, mb, ro = torch.bfloat16, 64, 32, 64, 8, 512
    cached = [c if c > 0 else 0 for c in E2E_CACHED]
    cu = cumsum0(E2E_NQ)
    total, maxq = cu[-1], max(E2E_NQ)
    kd, vd = descales(gen), descales(gen)
    kp, vp, bt = e2e_pool(gen, dtype, D, page, mb, kd, vd)
    for p in (kp, vp):
        p.view(torch.uint8)[p.view(torch.uint8) == 0x7F] = 0x38
    cos, sin = (t.to(DEV) for t in tables(ro, rd, torch.float32))
    steps = [packed_qkv(gen, total, D, dtype).to(DEV) for _ in range(2)]
    kp_d, vp_d, btd, kdd, vdd, cud = kp.to(DEV), vp.to(DEV), bt.to(DEV), kd.to(DEV), vd.to(DEV), i32(cu)
    lens_d, lens_now = i32(cached), i32([c + n for c, n in zip(cached, E2E_NQ)])
    qkv_s = steps[0].clone()

    def step(qkv, kpool, vpool, lens, now):
        q, k, v = split(qkv)
        tfa.kvcache_append_varlen(k, v, kpool, vpool, cud, lens, btd, rotary_cos=cos, rotary_sin=sin, q=q, k_descale=kdd, v_descale=vdd)
        torch.add(lens, torch.diff(cud), out=now)
        return tfa.flash_attn_with_kvcache(q, kpool, vpool, cache_seqlens=now, block_table=btd, causal=True, cu_seqlens_q=cud, max_seqlen_q=maxq, num_splits=1,
                                           k_descale=kdd, v_descale=vdd, return_softmax_lse=True)

    step(qkv_s, kp_d, vp_d, lens_d, lens_now)                                      # the warm-up, outside the capture: step 0 is in the pool
    torch.cuda.synchronize()
    qkv_s.copy_(steps[0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_s, lse_s = step(qkv_s, kp_d, vp_d, lens_d, lens_now)
    qkv_s.copy_(steps[1])                                                          # the next step's rows, the lengths advanced in place
    lens_d.add_(torch.diff(cud))
    kp_e, vp_e, lens_e, now_e, qkv_e = kp_d.clone(), vp_d.clone(), lens_d.clone(), lens_now.clone(), steps[1].clone()
    g.replay()
    torch.cuda.synchronize()
    out_e, lse_e = step(qkv_e, kp_e, vp_e, lens_e, now_e)
    torch.cuda.synchronize()
    assert lens_e.tolist() == [c + n for c, n in zip(cached, E2E_NQ)]
    assert torch.equal(raw(kp_d), raw(kp_e)) and torch.equal(raw(vp_d), raw(vp_e)), "the replayed append left other bytes than the eager one"
    assert not torch.equal(raw(kp_d), raw(kp.to(DEV))) and torch.equal(raw(qkv_s), raw(qkv_e)) and not torch.equal(raw(qkv_s), raw(steps[1]))
    assert torch.equal(raw(out_s), raw(out_e)) and torch.equal(lse_s.cpu(), lse_e.cpu())
    assert not torch.isnan(out_s.float()).any()
