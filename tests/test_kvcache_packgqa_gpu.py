"""GPU tests of ``flash_attn_with_kvcache(pack_gqa=)`` (tfa_fwd_kvcache_pack): the packed form of the KV-cache kernel at Nq > 1 — the Nq * G rows (position t,
head g) of a K/V head as position-major rows of one problem — against the fp64 reference of tests/test_kvcache_gpu.py, with that file's bars and input
distributions (q std 1.0, K/V std 0.5; 16-bit out |d| <= 1e-2, LSE |d| <= 1e-4 * max(1, |ref|), +inf exactly on rows that see no key): the packed rows run the
same arithmetic over the same keys.  Per-position causal masks, G not a power of two and MQA, more than one query block, paged and fp8 caches, the append, a
captured step, rows at and beyond Nq * G (never loaded into a result, never stored), Nq == 1's unchanged bits, determinism.  Every case compares every element."""
import ctypes as C
import math

import pytest
import torch

import tiny_flash_attention_amd as tfa
from tiny_flash_attention_amd import _lib, ops

pytestmark = pytest.mark.gpu

OUT_BAR = 1e-2
LSE_BAR = 1e-4
DEV = "cuda:0"
E4M3 = torch.float8_e4m3fn


# ---- the reference, the comparison and the page scatter of tests/test_kvcache_gpu.py (descales as in tests/test_kvcache_fp8_gpu.py) ---------------------------
def gather_cache(cache, block_table, b, n):
    """Keys [0, n) of sequence b as (n, Hk, D): rows of the contiguous cache, or of its pages in block-table order."""
    if block_table is None:
        return cache[b, :n]
    page = cache.shape[1]
    pages = [cache[int(block_table[b, i])] for i in range((n + page - 1) // page)]
    return torch.cat(pages, 0)[:n] if pages else cache[0, :0]


def reference(q, k_cache, v_cache, lens, block_table, scale, causal, kd=None, vd=None):
    """fp64 attention of every sequence over its own (decoded, descaled) keys: out (B, Nq, H, D), lse (B, H, Nq); rows that see no key: out = 0, lse = +inf."""
    q, k_cache, v_cache = q.double().cpu(), k_cache.cpu().double(), v_cache.cpu().double()
    bt = None if block_table is None else block_table.cpu()
    B, Nq, H, D = q.shape
    Hk = k_cache.shape[2]
    G = H // Hk
    kd = torch.ones(B, Hk, dtype=torch.float64) if kd is None else kd.double().cpu()
    vd = torch.ones(B, Hk, dtype=torch.float64) if vd is None else vd.double().cpu()
    out = torch.zeros(B, Nq, H, D, dtype=torch.float64)
    lse = torch.full((B, H, Nq), math.inf, dtype=torch.float64)
    for b in range(B):
        n = int(lens[b])
        if n == 0:
            continue
        k = (gather_cache(k_cache, bt, b, n) * kd[b].view(1, Hk, 1)).repeat_interleave(G, dim=1)          # (n, H, D)
        v = (gather_cache(v_cache, bt, b, n) * vd[b].view(1, Hk, 1)).repeat_interleave(G, dim=1)
        s = torch.einsum("qhd,khd->hqk", q[b], k) * scale                         # (H, Nq, n)
        if causal:
            i = torch.arange(Nq).view(Nq, 1)
            j = torch.arange(n).view(1, n)
            s = s.masked_fill(j > i + (n - Nq), -math.inf)
        l = torch.logsumexp(s, dim=-1)                                            # -inf where a row sees no key
        seen = torch.isfinite(l)
        p = torch.exp(s - torch.where(seen, l, torch.zeros_like(l)).unsqueeze(-1))
        p = torch.where(seen.unsqueeze(-1), p, torch.zeros_like(p))
        out[b] = torch.einsum("hqk,khd->qhd", p, v)
        lse[b] = torch.where(seen, l, torch.full_like(l, math.inf))
    return out, lse


def assert_matches(out, lse, ref_out, ref_lse, what=""):
    out, lse = out.double().cpu(), lse.double().cpu()
    assert out.shape == ref_out.shape and lse.shape == ref_lse.shape
    assert not torch.isnan(out).any(), f"{what}: NaN in out"
    assert not torch.isnan(lse).any(), f"{what}: NaN in lse"
    err = (out - ref_out).abs().max().item()
    inf_ref = torch.isinf(ref_lse)
    assert torch.equal(torch.isinf(lse) & (lse > 0), inf_ref), f"{what}: lse = +inf on other rows than the reference"
    fin = ~inf_ref
    rel = ((lse[fin] - ref_lse[fin]).abs() / ref_lse[fin].abs().clamp(min=1.0)).max().item() if fin.any() else 0.0
    print(f"{what}: max|d out| = {err:.3e} (bar {OUT_BAR}), max LSE err = {rel:.3e} (bar {LSE_BAR}), empty rows = {int(inf_ref.sum())}")
    assert err <= OUT_BAR, f"{what}: max|d out| = {err}"
    assert rel <= LSE_BAR, f"{what}: LSE error {rel}"
    if inf_ref.any():
        assert (out.transpose(1, 2)[inf_ref] == 0).all(), f"{what}: out != 0 on rows that see no key"


def randn(gen, *shape, dtype, std=0.5):
    return (torch.randn(*shape, generator=gen, dtype=torch.float32) * std).to(dtype)


def make_paged(gen, kc, vc, page, spare=3, fill=None):
    """Scatter a contiguous (B, cap, Hk, D) cache into pages through a seeded shuffled block table; no page is shared; `spare` unused pages hold garbage
    (or `fill`).  Works on the bytes, so 16-bit and e4m3 caches alike."""
    B, cap, Hk, D = kc.shape
    mb = cap // page
    nb = B * mb + spare
    perm = torch.randperm(nb, generator=gen)[: B * mb].view(B, mb)
    if kc.dtype == E4M3:
        kp = torch.full((nb, page, Hk, D), 0x7F, dtype=torch.uint8).view(E4M3)    # the NaN code
        vp = torch.full((nb, page, Hk, D), 0x7F, dtype=torch.uint8).view(E4M3)
    else:
        kp = randn(gen, nb, page, Hk, D, dtype=kc.dtype, std=3.0)
        vp = randn(gen, nb, page, Hk, D, dtype=kc.dtype, std=3.0)
        if fill is not None:
            kp[:] = fill
            vp[:] = fill
    raw = torch.uint8 if kc.dtype == E4M3 else torch.int16
    for b in range(B):
        for i in range(mb):
            kp.view(raw)[perm[b, i]] = kc.view(raw)[b, i * page:(i + 1) * page]
            vp.view(raw)[perm[b, i]] = vc.view(raw)[b, i * page:(i + 1) * page]
    return kp, vp, perm.to(torch.int32)


def run(q, kc, vc, lens, bt=None, k=None, v=None, causal=False, splits=0, scale=None, pack=True, kd=None, vd=None):
    d = lambda t: None if t is None else t.to(DEV)
    out, lse = tfa.flash_attn_with_kvcache(d(q), d(kc), d(vc), d(k), d(v), cache_seqlens=d(lens), block_table=d(bt), softmax_scale=scale, causal=causal,
                                           num_splits=splits, return_softmax_lse=True, pack_gqa=pack, k_descale=d(kd), v_descale=d(vd))
    torch.cuda.synchronize()
    return out, lse


def both_arms(q, kc, vc, lens, ref, what, bt=None, causal=False, splits=(1, 3), **kw):
    """pack_gqa=True and the same call with False at every split count, each against the reference; prints the largest difference between the arms."""
    scale = 1.0 / math.sqrt(q.shape[-1])
    for s in splits:
        out, lse = run(q, kc, vc, lens, bt, causal=causal, splits=s, scale=scale, pack=True, **kw)
        assert_matches(out, lse, *ref, what=f"{what} pack_gqa=True splits{s}")
        off, lse_off = run(q, kc, vc, lens, bt, causal=causal, splits=s, scale=scale, pack=False, **kw)
        assert_matches(off, lse_off, *ref, what=f"{what} pack_gqa=False splits{s}")
        print(f"{what} splits{s}: max|True - False| = {(out.float() - off.float()).abs().max().item():.3e}")


# ---- 1. positions ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [64, 128, 40])
@pytest.mark.parametrize("Nq", [2, 3, 5])
def test_positions(dtype, D, Nq):
    """G = 4: row r of the packed block is position r // 4 of head r % 4; lengths a multiple of 64, a non-multiple, 1 (rows that see no key, and — the last
    position — one that sees one key), 0 and the capacity."""
    gen = torch.Generator().manual_seed(1000 + 10 * D + Nq)
    B, H, Hk, cap = 5, 8, 2, 1024
    lens = torch.tensor([512, 700, 1, 0, 1024], dtype=torch.int32)
    q = randn(gen, B, Nq, H, D, dtype=dtype, std=1.0)
    kc, vc = randn(gen, B, cap, Hk, D, dtype=dtype), randn(gen, B, cap, Hk, D, dtype=dtype)
    scale = 1.0 / math.sqrt(D)
    for causal in (True, False):
        ref = reference(q, kc, vc, lens, None, scale, causal)
        if causal:                                                               # len 1: only the last position sees a key (exactly one)
            assert torch.isinf(ref[1][2, :, : Nq - 1]).all() and torch.isfinite(ref[1][2, :, Nq - 1]).all()
        both_arms(q, kc, vc, lens, ref, f"positions {dtype} D{D} Nq{Nq} causal={causal}", causal=causal)


# ---- 2. G that is no power of two, and MQA ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Hk", [(12, 4), (8, 1)])
def test_group_sizes_three_and_mqa(H, Hk):
    gen = torch.Generator().manual_seed(2000 + H)
    dtype, B, D, cap, Nq = torch.bfloat16, 4, 128, 1024, 4
    lens = torch.tensor([1000, 3, 130, 64], dtype=torch.int32)                   # one sequence shorter than Nq
    q = randn(gen, B, Nq, H, D, dtype=dtype, std=1.0)
    kc, vc = randn(gen, B, cap, Hk, D, dtype=dtype), randn(gen, B, cap, Hk, D, dtype=dtype)
    ref = reference(q, kc, vc, lens, None, 1.0 / math.sqrt(D), True)
    both_arms(q, kc, vc, lens, ref, f"H{H} Hk{Hk} Nq{Nq}", causal=True)


# ---- 3. more than one query block ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nq", [40, 33])
@pytest.mark.parametrize("causal", [True, False])
def test_more_than_one_query_block(Nq, causal):
    """H16 Hk4: 160 rows are two full-ish blocks (causal: the pair of a heavy and a light block in one workgroup), 132 rows a second block of 4 rows."""
    gen = torch.Generator().manual_seed(3000 + Nq)
    dtype, B, H, Hk, D, cap = torch.float16, 3, 16, 4, 64, 1024
    lens = torch.tensor([1024, 20, 300], dtype=torch.int32)                      # 20 < Nq: the first positions see nothing
    q = randn(gen, B, Nq, H, D, dtype=dtype, std=1.0)
    kc, vc = randn(gen, B, cap, Hk, D, dtype=dtype), randn(gen, B, cap, Hk, D, dtype=dtype)
    ref = reference(q, kc, vc, lens, None, 1.0 / math.sqrt(D), causal)
    if causal:
        assert torch.isinf(ref[1][1, :, : Nq - 20]).all() and torch.isfinite(ref[1][1, :, Nq - 20:]).all()
    both_arms(q, kc, vc, lens, ref, f"two blocks Nq{Nq} causal={causal}", causal=causal, splits=(1, 2))


# ---- 4. paged --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page", [64, 256])
def test_paged_matches_reference_and_contiguous_bits(page):
    gen = torch.Generator().manual_seed(4000 + page)
    dtype, B, H, Hk, D, cap, Nq = torch.bfloat16, 4, 8, 2, 128, 1024, 3
    lens = torch.tensor([1024, 333, 640, 65], dtype=torch.int32)
    q = randn(gen, B, Nq, H, D, dtype=dtype, std=1.0)
    kc, vc = randn(gen, B, cap, Hk, D, dtype=dtype), randn(gen, B, cap, Hk, D, dtype=dtype)
    kp, vp, bt = make_paged(gen, kc, vc, page)
    scale = 1.0 / math.sqrt(D)
    ref = reference(q, kp, vp, lens, bt, scale, True)
    for splits in (1, 3):
        out, lse = run(q, kp, vp, lens, bt, causal=True, splits=splits, scale=scale)
        assert_matches(out, lse, *ref, what=f"paged{page} splits{splits}")
        out_c, lse_c = run(q, kc, vc, lens, None, causal=True, splits=splits, scale=scale)
        assert torch.equal(out, out_c) and torch.equal(lse, lse_c), "paged and contiguous packed results differ in bits"


# ---- 5. nothing behind the length is read; rows at and beyond Nq * G are neither loaded into a result nor stored -------------------------------
CANARY = 0x7B7B


@pytest.mark.parametrize("paged", [False, True])
def test_nan_behind_the_lengths_and_canaries_around_q_and_out(paged):
    gen = torch.Generator().manual_seed(5)
    dtype, B, H, Hk, D, cap, Nq = torch.bfloat16, 3, 8, 2, 128, 1024, 4
    lens = torch.tensor([300, 64, 1000], dtype=torch.int32)
    q = randn(gen, B, Nq, H, D, dtype=dtype, std=1.0)
    kc, vc = randn(gen, B, cap, Hk, D, dtype=dtype), randn(gen, B, cap, Hk, D, dtype=dtype)
    scale = 1.0 / math.sqrt(D)
    ref = reference(q, kc, vc, lens, None, scale, True)
    for b in range(B):
        kc[b, int(lens[b]):] = float("nan")
        vc[b, int(lens[b]):] = float("nan")
    bt = None
    if paged:
        kc, vc, bt = make_paged(gen, kc, vc, 128, fill=float("nan"))             # the spare pages too
    # q: a slice of a larger NaN-filled buffer (16 packed rows of 128 in the block: the other 112 would be read from here or from the rows of other heads)
    pad = 64 * H * D
    q_whole = torch.full((pad + q.numel() + pad,), float("nan"), dtype=dtype, device=DEV)
    q_dev = q_whole[pad:pad + q.numel()].view(q.shape)
    q_dev.copy_(q)
    kc_d, vc_d, lens_d = kc.to(DEV), vc.to(DEV), lens.to(DEV)
    bt_d = None if bt is None else bt.to(DEV)
    for splits in (1, 3):
        out, lse = tfa.flash_attn_with_kvcache(q_dev, kc_d, vc_d, cache_seqlens=lens_d, block_table=bt_d, causal=True, num_splits=splits, return_softmax_lse=True,
                                               pack_gqa=True)
        torch.cuda.synchronize()
        assert not torch.isnan(out).any() and not torch.isnan(lse).any()
        assert_matches(out, lse, *ref, what=f"NaN behind the lengths paged={paged} splits{splits}")
    # out: the explicit C-ABI call into a buffer laid out like q, (B, Nq, H, D), with canary rows in front and behind — one chunk takes any out strides
    o_whole = torch.full((pad + q.numel() + pad,), CANARY, dtype=torch.int16, device=DEV)
    o_dev = o_whole[pad:pad + q.numel()].view(dtype).view(B, Nq, H, D)
    lse_whole = torch.full((64 + B * H * Nq + 64,), -7.0, dtype=torch.float32, device=DEV)
    lse_dev = lse_whole[64:64 + B * H * Nq].view(B, H, Nq)
    p = ops._kvcache_params(q_dev, kc_d, vc_d, o_dev.transpose(1, 2), lse_dev, lens_d, bt_d, None, None, scale, True)
    L = _lib.lib()
    with torch.cuda.device(q_dev.device):
        _lib.check(L.tfa_fwd_kvcache_pack(C.byref(p), None, _lib.TFA_PACK_GQA_ON, 1, None, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert_matches(o_dev, lse_dev, *ref, what=f"C ABI, out laid out like q, paged={paged}")
    w = o_whole.cpu()
    assert (w[:pad] == CANARY).all() and (w[pad + q.numel():] == CANARY).all(), "a canary around out was overwritten"
    lw = lse_whole.cpu()
    assert (lw[:64] == -7.0).all() and (lw[64 + B * H * Nq:] == -7.0).all(), "a canary around lse was overwritten"
    qw = q_whole.cpu()
    assert torch.isnan(qw[:pad]).all() and torch.isnan(qw[pad + q.numel():]).all() and torch.equal(q_dev.cpu(), q), "q or its surroundings were written"


# ---- 6. fp8 cache ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged", [False, True])
def test_fp8_cache(paged):
    gen = torch.Generator().manual_seed(6)
    dtype, B, H, Hk, D, cap, Nq = torch.bfloat16, 3, 8, 2, 128, 1024, 4
    lens = torch.tensor([1024, 2, 515], dtype=torch.int32)                       # 2 < Nq
    q = randn(gen, B, Nq, H, D, dtype=dtype, std=1.0)
    kd = 0.002 + 0.018 * torch.rand(B, Hk, generator=gen, dtype=torch.float32)
    vd = 0.002 + 0.018 * torch.rand(B, Hk, generator=gen, dtype=torch.float32)
    quant = lambda x, d: (x.float() / d.view(B, 1, Hk, 1)).clamp(-448.0, 448.0).to(E4M3)
    k8 = quant(randn(gen, B, cap, Hk, D, dtype=torch.float32), kd)
    v8 = quant(randn(gen, B, cap, Hk, D, dtype=torch.float32), vd)
    for b in range(B):                                                            # the NaN code behind every length
        k8.view(torch.uint8)[b, int(lens[b]):] = 0x7F
        v8.view(torch.uint8)[b, int(lens[b]):] = 0x7F
    scale = 1.0 / math.sqrt(D)
    ref = reference(q, k8, v8, lens, None, scale, True, kd, vd)
    k16, v16 = k8.to(dtype), v8.to(dtype)                                         # exact: every finite e4m3 value is a bf16
    bt = None
    kk, vv = k8, v8
    if paged:
        state = gen.get_state()
        kk, vv, bt = make_paged(gen, k8, v8, 128)
        gen.set_state(state)
        k16, v16, bt16 = make_paged(gen, k16, v16, 128, fill=float("nan"))
        assert torch.equal(bt, bt16)
    for splits in (1, 3):
        out, lse = run(q, kk, vv, lens, bt, causal=True, splits=splits, scale=scale, kd=kd, vd=vd)
        assert_matches(out, lse, *ref, what=f"fp8 paged={paged} splits{splits}")
        # descales of 1.0: the decoded values are x / descale, hundreds in magnitude — no case for the bar of std-0.5 inputs, but the bits are the 16-bit call's
        one, lse_one = run(q, kk, vv, lens, bt, causal=True, splits=splits, scale=scale)
        out16, lse16 = run(q, k16, v16, lens, bt, causal=True, splits=splits, scale=scale)
        assert torch.equal(one, out16) and torch.equal(lse_one, lse16), "fp8 at descale 1.0 and the 16-bit packed call over the converted caches differ in bits"


# ---- 7. append -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged", [False, True])
def test_append_then_packed_attention(paged):
    gen = torch.Generator().manual_seed(7)
    dtype, B, H, Hk, D, cap, page, Nq = torch.float16, 4, 8, 2, 64, 512, 128, 3
    lens = torch.tensor([100, cap - Nq, 0, 255], dtype=torch.int32)
    q = randn(gen, B, Nq, H, D, dtype=dtype, std=1.0)
    kc, vc = randn(gen, B, cap, Hk, D, dtype=dtype), randn(gen, B, cap, Hk, D, dtype=dtype)
    kn, vn = randn(gen, B, Nq, Hk, D, dtype=dtype), randn(gen, B, Nq, Hk, D, dtype=dtype)
    bt = None
    if paged:
        kc, vc, bt = make_paged(gen, kc, vc, page)
    ke, ve = kc.clone(), vc.clone()
    for b in range(B):
        for t in range(Nq):
            pos = int(lens[b]) + t
            where = (int(bt[b, pos // page]), pos % page) if paged else (b, pos)
            ke[where] = kn[b, t]
            ve[where] = vn[b, t]
    scale = 1.0 / math.sqrt(D)
    ref = reference(q, ke, ve, lens + Nq, bt, scale, True)
    lens_d = lens.to(DEV)
    for splits in (1, 2):
        k_dev, v_dev = kc.to(DEV), vc.to(DEV)
        out, lse = tfa.flash_attn_with_kvcache(q.to(DEV), k_dev, v_dev, kn.to(DEV), vn.to(DEV), cache_seqlens=lens_d, block_table=None if bt is None else bt.to(DEV),
                                               causal=True, num_splits=splits, return_softmax_lse=True, pack_gqa=True)
        torch.cuda.synchronize()
        assert torch.equal(lens_d.cpu(), lens), "cache_seqlens was modified"
        assert torch.equal(k_dev.cpu().view(torch.int16), ke.view(torch.int16)) and torch.equal(v_dev.cpu().view(torch.int16), ve.view(torch.int16)), \
            "the cache does not hold the new rows"
        assert_matches(out, lse, *ref, what=f"append paged={paged} splits{splits}")


# ---- 8. a captured packed step ---------------------------------------------------------------------------------------------------------------
def test_captured_packed_step_replays_with_advanced_lengths():
    gen = torch.Generator().manual_seed(8)
    dtype, B, H, Hk, D, cap, page, Nq = torch.bfloat16, 3, 8, 2, 128, 1024, 256, 2
    lens = torch.tensor([1000, 17, 0], dtype=torch.int32)
    kc, vc = randn(gen, B, cap, Hk, D, dtype=dtype), randn(gen, B, cap, Hk, D, dtype=dtype)
    kc, vc, bt = make_paged(gen, kc, vc, page)
    steps = [(randn(gen, B, Nq, H, D, dtype=dtype, std=1.0), randn(gen, B, Nq, Hk, D, dtype=dtype), randn(gen, B, Nq, Hk, D, dtype=dtype)) for _ in range(3)]
    k_dev, v_dev, lens_dev, bt_dev = kc.to(DEV), vc.to(DEV), lens.to(DEV), bt.to(DEV)
    q_s, k_s, v_s = (t.to(DEV).clone() for t in steps[0])
    call = lambda: tfa.flash_attn_with_kvcache(q_s, k_dev, v_dev, k_s, v_s, cache_seqlens=lens_dev, block_table=bt_dev, causal=True, num_splits=2,
                                               return_softmax_lse=True, pack_gqa=True)
    call()                                                                        # one warm-up call outside the capture (it appends step 0's rows)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                                     # append, attention, merge on one stream: a straight line
        out_s, lse_s = call()
    scale = 1.0 / math.sqrt(D)
    kc_cpu, vc_cpu, cur = kc.clone(), vc.clone(), lens.clone()
    for r in range(3):
        qr, kr, vr = steps[r]
        q_s.copy_(qr.to(DEV))
        k_s.copy_(kr.to(DEV))
        v_s.copy_(vr.to(DEV))
        g.replay()
        torch.cuda.synchronize()
        for b in range(B):                                                        # the CPU mirror of the append
            for t in range(Nq):
                pos = int(cur[b]) + t
                kc_cpu[int(bt[b, pos // page]), pos % page] = kr[b, t]
                vc_cpu[int(bt[b, pos // page]), pos % page] = vr[b, t]
        ref = reference(qr, kc_cpu, vc_cpu, cur + Nq, bt, scale, True)
        assert_matches(out_s, lse_s, *ref, what=f"replay {r}")
        lens_dev.add_(Nq)                                                         # the caller advances the lengths, in place on the device
        cur = cur + Nq
    torch.cuda.synchronize()


# ---- 9. one row per sequence keeps its bits -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splits", [1, 4])
def test_one_row_keeps_its_bits_and_false_unpacks_it(splits):
    gen = torch.Generator().manual_seed(9)
    dtype, B, H, Hk, D, cap = torch.bfloat16, 3, 16, 2, 128, 1024
    lens = torch.tensor([1024, 777, 64], dtype=torch.int32)
    q = randn(gen, B, 1, H, D, dtype=dtype, std=1.0)
    kc, vc = randn(gen, B, cap, Hk, D, dtype=dtype), randn(gen, B, cap, Hk, D, dtype=dtype)
    scale = 1.0 / math.sqrt(D)
    ref = reference(q, kc, vc, lens, None, scale, True)
    on, lse_on = run(q, kc, vc, lens, causal=True, splits=splits, scale=scale, pack=True)
    auto, lse_auto = run(q, kc, vc, lens, causal=True, splits=splits, scale=scale, pack=None)
    assert torch.equal(on, auto) and torch.equal(lse_on, lse_auto), "pack_gqa=True at Nq == 1 is not the call pack_gqa=None runs"
    assert_matches(on, lse_on, *ref, what=f"Nq1 True splits{splits}")
    off, lse_off = run(q, kc, vc, lens, causal=True, splits=splits, scale=scale, pack=False)
    assert_matches(off, lse_off, *ref, what=f"Nq1 False splits{splits}")


# ---- 10. determinism -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splits", [1, 3])
def test_two_packed_calls_are_bit_equal(splits):
    gen = torch.Generator().manual_seed(10)
    dtype, B, H, Hk, D, cap, Nq = torch.float16, 3, 8, 2, 64, 1024, 5
    lens = torch.tensor([1024, 4, 513], dtype=torch.int32)
    q = randn(gen, B, Nq, H, D, dtype=dtype, std=1.0)
    kc, vc = randn(gen, B, cap, Hk, D, dtype=dtype), randn(gen, B, cap, Hk, D, dtype=dtype)
    a, la = run(q, kc, vc, lens, causal=True, splits=splits)
    b, lb = run(q, kc, vc, lens, causal=True, splits=splits)
    assert torch.equal(a, b) and torch.equal(la.view(torch.int32), lb.view(torch.int32)), "two runs of the same packed call differ"
