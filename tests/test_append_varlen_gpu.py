"""GPU tests of ``kvcache_append_varlen`` (tfa_kvcache_append_varlen) and of the two serving steps it completes.

The append: the WHOLE pool is compared as int16 bits against a pool built on the CPU; the pool is pre-filled with a sentinel pattern that includes NaN bits, so a
stray store anywhere shows up.  End to end (bars of include/tfa.h: 16-bit out |d| <= 1e-2, LSE |d| <= 1e-4 relative): a unified batch — append, then
flash_attn_varlen_func(block_table=) — and a captured decode step — apply_rotary_emb_qk_, then flash_attn_with_kvcache(k=, v=) — against fp64 attention written here,
with the rotary embedding applied in the reference (fp64, rounded once to the 16-bit type: FlashAttention-2's rotary KV-cache semantics — q at the position of
its row, k at its key position, the cache holding rotated keys)."""
import math

import pytest
import torch

import tiny_flash_attention_amd as tfa
from tiny_flash_attention_amd import ops
from rotary_ref import packed_positions, rotary_ref64, tables

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OUT_BAR, LSE_BAR = 1e-2, 1e-4
B, HK = 4, 2
CACHED = [0, 63, 64, 130]
NEW = [0, 1, 3, 70]                      # the 70 crosses a page boundary and a table entry
PAD = 3                                  # padding rows behind cu[B]
DTYPES = [torch.bfloat16, torch.float16]


def cumsum0(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return cu


def randn(gen, *shape, dtype, std=0.5):
    return (torch.randn(*shape, generator=gen, dtype=torch.float32) * std).to(dtype)


def sentinel(shape, dtype):
    """A pool full of a bit pattern that no append produces by accident; every fifth element holds NaN bits (0x7fff in both types)."""
    n = math.prod(shape)
    bits = ((torch.arange(n, dtype=torch.int64) * 40503 + 12345) % 65536 - 32768).to(torch.int16)
    bits[::5] = 0x7FFF
    return bits.view(shape).view(dtype)


def bits(t):
    return t.contiguous().view(torch.int16).cpu()


def packed_kv(gen, total, D, dtype, heads=2):
    """k, v (total, HK, D) as slices of one packed projection (total, heads + 2 HK, D)."""
    qkv = randn(gen, total, heads + 2 * HK, D, dtype=dtype)
    return qkv, qkv[:, heads:heads + HK], qkv[:, heads + HK:]


def shuffled_table(gen, mb, spare=3):
    nb = B * mb + spare
    return nb, torch.randperm(nb, generator=gen)[: B * mb].view(B, mb).to(torch.int32)


def expected_pool(pool, rows, cu, cached, bt, page, cap):
    """The CPU mirror of the append into a (num_pages, page, HK, D) pool — or, bt None, a (B, cap, HK, D) cache: drops as the header states them."""
    want = pool.clone()
    for b in range(len(cached)):
        for t in range(cu[b + 1] - cu[b]):
            pos = cached[b] + t
            if pos < 0 or pos >= cap:
                continue
            if bt is None:
                want[b, pos] = rows[cu[b] + t]
                continue
            pg = int(bt[b, pos // page])
            if 0 <= pg < pool.shape[0]:
                want[pg, pos % page] = rows[cu[b] + t]
    return want


def append(k, v, kp, vp, cu, cached, bt, **kw):
    d = lambda t: None if t is None else t.to(DEV)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=DEV)
    assert tfa.kvcache_append_varlen(k, v, kp, vp, i32(cu), i32(cached), d(bt), **kw) is None
    torch.cuda.synchronize()


@pytest.mark.parametrize("layout", ["pages_rows_heads", "pages_heads_rows"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [64, 40])
@pytest.mark.parametrize("page", [64, 128])
def test_paged_pool_bits(page, D, dtype, layout):
    gen = torch.Generator().manual_seed(page + D)
    cu = cumsum0(NEW)
    total = cu[-1] + PAD
    qkv, k, v = packed_kv(gen, total, D, dtype)
    mb = 256 // page
    nb, bt = shuffled_table(gen, mb)
    kp0, vp0 = sentinel((nb, page, HK, D), dtype), sentinel((nb, page, HK, D), dtype).roll(1, 0)
    want_k, want_v = (expected_pool(p, r, cu, CACHED, bt, page, mb * page) for p, r in ((kp0, k), (vp0, v)))
    qkv_d = qkv.to(DEV)
    if layout == "pages_heads_rows":                                            # a (num_pages, HK, page, D) pool viewed as (num_pages, page, HK, D)
        kp, vp = (p.transpose(1, 2).contiguous().to(DEV).transpose(1, 2) for p in (kp0, vp0))
        assert kp.stride(1) == D and kp.stride(2) == page * D
    else:
        kp, vp = kp0.to(DEV), vp0.to(DEV)
    append(qkv_d[:, 2:2 + HK], qkv_d[:, 2 + HK:], kp, vp, cu, CACHED, bt)
    assert torch.equal(bits(kp), bits(want_k)), "k pool differs from the pool built on the CPU"
    assert torch.equal(bits(vp), bits(want_v)), "v pool differs from the pool built on the CPU"
    assert torch.equal(bits(qkv_d), bits(qkv)), "the new rows were modified"
    assert not torch.equal(bits(want_k), bits(kp0))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cap", [256, 192])
def test_contiguous_cache_and_rows_past_the_capacity(cap, dtype):
    """(B, capacity, HK, D) without a table; capacity 192: the last sequence (130 cached + 70 new) loses exactly its rows at positions 192 .. 199."""
    gen = torch.Generator().manual_seed(cap)
    D, cu = 64, cumsum0(NEW)
    total = cu[-1] + PAD
    qkv, k, v = packed_kv(gen, total, D, dtype)
    kc0, vc0 = sentinel((B, 2 * cap, HK, D), dtype)[:, :cap], sentinel((B, cap, HK, D), dtype).roll(3, 1)      # k: a strided view, sequences 2 * cap rows apart
    want_k, want_v = (expected_pool(p, r, cu, CACHED, None, 0, cap) for p, r in ((kc0, k), (vc0, v)))
    whole = sentinel((B, 2 * cap, HK, D), dtype).to(DEV)
    kc, vc = whole[:, :cap], vc0.to(DEV)
    qkv_d = qkv.to(DEV)
    append(qkv_d[:, 2:2 + HK], qkv_d[:, 2 + HK:], kc, vc, cu, CACHED, None)
    assert torch.equal(bits(kc), bits(want_k)) and torch.equal(bits(vc), bits(want_v))
    assert torch.equal(bits(whole[:, cap:]), bits(sentinel((B, 2 * cap, HK, D), dtype)[:, cap:])), "rows behind the capacity were written"
    written = (bits(want_k) != bits(kc0)).any(-1).any(-1).sum().item()
    assert written == sum(min(n, max(0, cap - c)) for n, c in zip(NEW, CACHED))


@pytest.mark.parametrize("dtype", DTYPES)
def test_capacity_and_bad_table_entries_drop_their_rows_and_nothing_else(dtype):
    """Paged, capacity 3 x 64 = 192: rows at positions >= 192 are dropped; a table entry of -1 and one of num_pages drop the rows that map to them."""
    gen = torch.Generator().manual_seed(9)
    page, mb, D, cu = 64, 3, 64, cumsum0(NEW)
    total = cu[-1] + PAD
    qkv, k, v = packed_kv(gen, total, D, dtype)
    nb, bt = shuffled_table(gen, mb)
    for bad in (None, (2, 1, -1), (3, 2, nb)):                                   # sequence 2 appends into block 1 (positions 64 .. 66), sequence 3 into block 2 (130 .. 191)
        table = bt.clone()
        if bad:
            table[bad[0], bad[1]] = bad[2]
        kp0, vp0 = sentinel((nb, page, HK, D), dtype), sentinel((nb, page, HK, D), dtype).roll(7, 1)
        want_k, want_v = (expected_pool(p, r, cu, CACHED, table, page, mb * page) for p, r in ((kp0, k), (vp0, v)))
        kp, vp, qkv_d = kp0.to(DEV), vp0.to(DEV), qkv.to(DEV)
        append(qkv_d[:, 2:2 + HK], qkv_d[:, 2 + HK:], kp, vp, cu, CACHED, table)
        assert torch.equal(bits(kp), bits(want_k)) and torch.equal(bits(vp), bits(want_v)), f"bad entry {bad}"
        written = (bits(want_k) != bits(kp0)).any(-1).any(-1).sum().item()
        assert written == {None: 0 + 1 + 3 + 62, (2, 1, -1): 1 + 62, (3, 2, nb): 1 + 3}[bad]


@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_equal_counts_leave_the_bits_of_flash_attn_with_kvcache(dtype, paged):
    gen = torch.Generator().manual_seed(4)
    n_new, D, H, page, cap = 3, 64, 4, 64, 256
    kn, vn = randn(gen, B, n_new, HK, D, dtype=dtype).to(DEV), randn(gen, B, n_new, HK, D, dtype=dtype).to(DEV)
    q = randn(gen, B, n_new, H, D, dtype=dtype).to(DEV)
    lens = torch.tensor(CACHED, dtype=torch.int32, device=DEV)
    if paged:
        nb, bt = shuffled_table(gen, cap // page)
        shape, bt = (nb, page, HK, D), bt.to(DEV)
    else:
        shape, bt = (B, cap, HK, D), None
    pools = [[sentinel(shape, dtype).to(DEV), sentinel(shape, dtype).roll(1, 0).to(DEV)] for _ in range(2)]
    tfa.flash_attn_with_kvcache(q, pools[0][0], pools[0][1], kn, vn, cache_seqlens=lens, block_table=bt, causal=True, num_splits=1)
    cu = torch.arange(B + 1, dtype=torch.int32, device=DEV) * n_new
    tfa.kvcache_append_varlen(kn.view(B * n_new, HK, D), vn.view(B * n_new, HK, D), pools[1][0], pools[1][1], cu, lens, bt)
    torch.cuda.synchronize()
    assert torch.equal(bits(pools[0][0]), bits(pools[1][0])) and torch.equal(bits(pools[0][1]), bits(pools[1][1]))
    assert not torch.equal(bits(pools[1][0]), bits(sentinel(shape, dtype)))


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_rotary_equals_rotating_first_and_appending_plain(dtype, interleaved):
    """The pool holds the bits apply_rotary_emb(k, cu_seqlens=cu, seqlen_offsets=cache_seqlens) + the plain append leave; V is copied; positions at and behind
    seqlen_ro (180: the last sequence reaches 199) are stored unrotated."""
    gen = torch.Generator().manual_seed(5)
    page, mb, ro, cu = 64, 4, 180, cumsum0(NEW)
    total = cu[-1] + PAD
    for D, rd, tdt in ((64, 64, dtype), (128, 32, torch.float32), (40, 16, dtype), (128, 128, dtype)):
        qkv, k, v = packed_kv(gen, total, D, dtype)
        qkv_d = qkv.to(DEV)
        kd, vd = qkv_d[:, 2:2 + HK], qkv_d[:, 2 + HK:]
        nb, bt = shuffled_table(gen, mb)
        cos, sin = (t.to(DEV) for t in tables(ro, rd, tdt))
        pools = [[sentinel((nb, page, HK, D), dtype).to(DEV), sentinel((nb, page, HK, D), dtype).roll(1, 0).to(DEV)] for _ in range(2)]
        cud, lens = torch.tensor(cu, dtype=torch.int32, device=DEV), torch.tensor(CACHED, dtype=torch.int32, device=DEV)
        k_rot = tfa.apply_rotary_emb(kd, cos, sin, interleaved=interleaved, cu_seqlens=cud, seqlen_offsets=lens)
        tfa.kvcache_append_varlen(k_rot, vd, pools[0][0], pools[0][1], cud, lens, bt.to(DEV))
        tfa.kvcache_append_varlen(kd, vd, pools[1][0], pools[1][1], cud, lens, bt.to(DEV), rotary_cos=cos, rotary_sin=sin, rotary_interleaved=interleaved)
        torch.cuda.synchronize()
        assert torch.equal(bits(pools[0][0]), bits(pools[1][0])), f"fused rotary differs from rotate-then-append (D {D}, rotary_dim {rd})"
        assert torch.equal(bits(pools[0][1]), bits(pools[1][1]))
        assert not torch.equal(bits(k_rot), bits(kd)) and torch.equal(bits(qkv_d), bits(qkv))
        want_v = expected_pool(sentinel((nb, page, HK, D), dtype).roll(1, 0), v, cu, CACHED, bt, page, mb * page)
        assert torch.equal(bits(pools[1][1]), bits(want_v))


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
def rope16(x, cos, sin, pos, interleaved, dtype):
    """The reference's rotary embedding: fp64, rounded once to the 16-bit type.  x (R, H, D), pos (R,)."""
    return rotary_ref64(x, cos, sin, pos, interleaved)[0].to(dtype)


def attend64(q, k, v, scale):
    """fp64 causal (bottom-right aligned) attention of one sequence: q (nq, H, D), k / v (n, HK, D) -> out (nq, H, D), lse (H, nq)."""
    q, k, v = q.double(), k.double(), v.double()
    nq, n, G = q.shape[0], k.shape[0], q.shape[1] // k.shape[1]
    k, v = k.repeat_interleave(G, dim=1), v.repeat_interleave(G, dim=1)
    s = torch.einsum("qhd,khd->hqk", q, k) * scale
    i, j = torch.arange(nq).view(nq, 1), torch.arange(n).view(1, n)
    s = s.masked_fill(j > i + (n - nq), -math.inf)
    lse = torch.logsumexp(s, dim=-1)
    return torch.einsum("hqk,khd->qhd", torch.exp(s - lse.unsqueeze(-1)), v), lse


def assert_close(out, lse, ref_out, ref_lse, what):
    err = (out.double().cpu() - ref_out).abs().max().item()
    rel = ((lse.double().cpu() - ref_lse).abs() / ref_lse.abs().clamp(min=1.0)).max().item()
    print(f"{what}: max|d out| = {err:.3e} (bar {OUT_BAR}), max LSE err = {rel:.3e} (bar {LSE_BAR})")
    assert err <= OUT_BAR and rel <= LSE_BAR, what


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_unified_batch_append_then_paged_varlen_attention(dtype, interleaved):
    """One chunked-prefill step: the cached keys are in the pool (rotated), the new rows are rotated and appended by one call, q is rotated at the positions of its rows,
    flash_attn_varlen_func(block_table=) attends.  Against fp64 attention over the same keys held contiguously with the rotary embedding applied in the reference, and
    — in bits — against the same attention over a pool filled by index_put_."""
    gen = torch.Generator().manual_seed(6)
    H, D, rd, page, mb, ro = 4, 64, 32, 64, 4, 256
    cu, cu_all = cumsum0(NEW), cumsum0([c + n for c, n in zip(CACHED, NEW)])
    total = cu[-1]
    q = randn(gen, total, H, D, dtype=dtype, std=1.0)
    k_all = [randn(gen, c + n, HK, D, dtype=dtype) for c, n in zip(CACHED, NEW)]         # raw keys of every sequence, cached and new
    v_all = [randn(gen, c + n, HK, D, dtype=dtype) for c, n in zip(CACHED, NEW)]
    cos, sin = tables(ro, rd, dtype)
    # the reference: rotated keys of every sequence, rotated queries, fp64 attention per sequence
    scale = 1.0 / math.sqrt(D)
    ref_out, ref_lse = torch.zeros(total, H, D, dtype=torch.float64), torch.zeros(H, total, dtype=torch.float64)
    k_rot = [rope16(k, cos, sin, torch.arange(k.shape[0]), interleaved, dtype) for k in k_all]
    for b in range(B):
        if NEW[b] == 0:
            continue
        qb = rope16(q[cu[b]:cu[b + 1]], cos, sin, CACHED[b] + torch.arange(NEW[b]), interleaved, dtype)
        o, l = attend64(qb, k_rot[b], v_all[b], scale)
        ref_out[cu[b]:cu[b + 1]], ref_lse[:, cu[b]:cu[b + 1]] = o, l
    # the device: a pool that holds the cached keys (the reference's rotated bits), then the step
    nb, bt = shuffled_table(gen, mb)
    kp, vp = sentinel((nb, page, HK, D), dtype), sentinel((nb, page, HK, D), dtype).roll(1, 0)
    for b in range(B):
        for pos in range(CACHED[b]):
            kp[int(bt[b, pos // page]), pos % page], vp[int(bt[b, pos // page]), pos % page] = k_rot[b][pos], v_all[b][pos]
    kp, vp, btd = kp.to(DEV), vp.to(DEV), bt.to(DEV)
    kp2, vp2 = kp.clone(), vp.clone()
    k_new = torch.cat([k[c:] for k, c in zip(k_all, CACHED)]).to(DEV)
    v_new = torch.cat([v[c:] for v, c in zip(v_all, CACHED)]).to(DEV)
    cud, cuk = torch.tensor(cu, dtype=torch.int32, device=DEV), torch.tensor(cu_all, dtype=torch.int32, device=DEV)
    lens, cd, sd = torch.tensor(CACHED, dtype=torch.int32, device=DEV), cos.to(DEV), sin.to(DEV)
    tfa.kvcache_append_varlen(k_new, v_new, kp, vp, cud, lens, btd, rotary_cos=cd, rotary_sin=sd, rotary_interleaved=interleaved)
    q_rot = tfa.apply_rotary_emb(q.to(DEV), cd, sd, interleaved=interleaved, cu_seqlens=cud, seqlen_offsets=lens)
    out, lse = ops.flash_attn_varlen_fwd(q_rot, kp, vp, cud, cuk, max(NEW), max(cu_all[i + 1] - cu_all[i] for i in range(B)), True, scale, block_table=btd)
    out_f = tfa.flash_attn_varlen_func(q_rot, kp, vp, cud, cuk, max(NEW), 200, causal=True, block_table=btd)
    torch.cuda.synchronize()
    assert_close(out, lse, ref_out, ref_lse, f"unified batch {dtype} interleaved={interleaved}")
    assert torch.equal(bits(out_f), bits(out))
    # the torch composition: rotate k with part 1, slot indices on the host, index_put_
    k_r = tfa.apply_rotary_emb(k_new, cd, sd, interleaved=interleaved, cu_seqlens=cud, seqlen_offsets=lens)
    pages, rows = [], []
    for b in range(B):
        for t in range(NEW[b]):
            pos = CACHED[b] + t
            pages.append(int(bt[b, pos // page]))
            rows.append(pos % page)
    idx = (torch.tensor(pages, device=DEV), torch.tensor(rows, device=DEV))
    kp2.index_put_(idx, k_r)
    vp2.index_put_(idx, v_new)
    out2, lse2 = ops.flash_attn_varlen_fwd(q_rot, kp2, vp2, cud, cuk, max(NEW), 200, True, scale, block_table=btd)
    torch.cuda.synchronize()
    assert torch.equal(bits(kp2), bits(kp)) and torch.equal(bits(vp2), bits(vp))
    assert torch.equal(bits(out2), bits(out)) and torch.equal(lse2.cpu(), lse.cpu())


@pytest.mark.parametrize("paged", [False, True])
def test_captured_decode_step_with_rotary_replays_at_advanced_positions(paged):
    """apply_rotary_emb_qk_ (seqlen_offsets = cache_seqlens) + flash_attn_with_kvcache(k=, v=), captured once, replayed after cache_seqlens was advanced in place and the
    static q / k / v buffers were refilled: every replay rotates at the new positions."""
    gen = torch.Generator().manual_seed(7)
    dtype, H, D, rd, cap, page = torch.bfloat16, 8, 128, 64, 512, 256
    lens = torch.tensor([500, 17, 255, 0], dtype=torch.int32)
    kc, vc = randn(gen, B, cap, HK, D, dtype=dtype), randn(gen, B, cap, HK, D, dtype=dtype)     # the cached keys: rotated long ago, any values
    cos, sin = tables(cap, rd, torch.float32)
    bt = None
    if paged:
        nb, bt = shuffled_table(gen, cap // page)
        kp, vp = sentinel((nb, page, HK, D), dtype), sentinel((nb, page, HK, D), dtype)
        for b in range(B):
            for i in range(cap // page):
                kp[int(bt[b, i])], vp[int(bt[b, i])] = kc[b, i * page:(i + 1) * page], vc[b, i * page:(i + 1) * page]
    steps = [(randn(gen, B, 1, H, D, dtype=dtype, std=1.0), randn(gen, B, 1, HK, D, dtype=dtype), randn(gen, B, 1, HK, D, dtype=dtype)) for _ in range(4)]
    k_dev, v_dev = (kp.to(DEV), vp.to(DEV)) if paged else (kc.to(DEV), vc.to(DEV))
    lens_dev, cd, sd = lens.to(DEV), cos.to(DEV), sin.to(DEV)
    bt_dev = None if bt is None else bt.to(DEV)
    q_s, k_s, v_s = (t.to(DEV).clone() for t in steps[0])

    def step():
        tfa.apply_rotary_emb_qk_(q_s, k_s, cd, sd, seqlen_offsets=lens_dev)
        return tfa.flash_attn_with_kvcache(q_s, k_dev, v_dev, k_s, v_s, cache_seqlens=lens_dev, block_table=bt_dev, causal=True, num_splits=1, return_softmax_lse=True)

    step()                                                                        # one warm-up call outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_s, lse_s = step()
    scale = 1.0 / math.sqrt(D)
    kc_cpu, vc_cpu, cur = kc.clone(), vc.clone(), lens.clone()
    for r in range(1, 4):
        qr, kr, vr = steps[r]
        q_s.copy_(qr.to(DEV))
        k_s.copy_(kr.to(DEV))
        v_s.copy_(vr.to(DEV))
        g.replay()
        torch.cuda.synchronize()
        ref_out, ref_lse = torch.zeros(B, 1, H, D, dtype=torch.float64), torch.zeros(B, H, 1, dtype=torch.float64)
        for b in range(B):
            pos = int(cur[b])
            kc_cpu[b, pos] = rope16(kr[b], cos, sin, torch.tensor([pos]), False, dtype)[0]
            vc_cpu[b, pos] = vr[b, 0]
            qb = rope16(qr[b], cos, sin, torch.tensor([pos]), False, dtype)
            ref_out[b], ref_lse[b] = attend64(qb, kc_cpu[b, :pos + 1], vc_cpu[b, :pos + 1], scale)
        assert_close(out_s, lse_s, ref_out, ref_lse, f"replay {r} paged={paged}")
        lens_dev.add_(1)                                                          # the caller advances the lengths, in place on the device
        cur = cur + 1
    torch.cuda.synchronize()
