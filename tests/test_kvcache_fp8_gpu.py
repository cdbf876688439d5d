"""GPU tests of the fp8 (e4m3) K/V cache of ``flash_attn_with_kvcache`` (tfa_fwd_kvcache_fp8, tfa_kvcache_append_fp8): ``k_cache`` / ``v_cache`` of dtype
``torch.float8_e4m3fn`` with one float32 descale per (sequence, K/V head).

The reference is written here and is the one of tests/test_kvcache_gpu.py run over the DEQUANTISED cache: for each sequence the keys [0, len_b) are gathered
through the block table, decoded — ``cache.double() * descale[b, hk]`` — and scores, causal mask at shift_b = len_b - Nq, logsumexp and P @ v are computed in fp64
on the CPU.  Bars (include/tfa.h): 16-bit out |d| <= 1e-2; LSE |d| <= 1e-4 * max(1, |ref|), +inf exactly on rows that see no key.  Every case compares every
output element.  Inputs: a std-0.5 tensor quantised with descales drawn per (b, hk) from [0.002, 0.02], so the dequantised K / V keep the std the 16-bit tests use
and outputs stay O(1), where the absolute bar means something."""
import math

import pytest
import torch

import tiny_flash_attention_amd as tfa

pytestmark = pytest.mark.gpu

OUT_BAR = 1e-2
LSE_BAR = 1e-4
DEV = "cuda:0"
E4M3 = torch.float8_e4m3fn
NAN_BYTE = 0x7F


def gather_cache(cache, block_table, b, n):
    """Keys [0, n) of sequence b as (n, Hk, D): rows of the contiguous cache, or of its pages in block-table order."""
    if block_table is None:
        return cache[b, :n]
    page = cache.shape[1]
    pages = [cache[int(block_table[b, i])] for i in range((n + page - 1) // page)]
    return torch.cat(pages, 0)[:n] if pages else cache[0, :0]


def reference(q, k8, v8, kd, vd, lens, block_table, scale, causal):
    """fp64 attention of every sequence over its own DECODED keys: out (B, Nq, H, D), lse (B, H, Nq); rows that see no key: out = 0, lse = +inf.
    k8 / v8: e4m3 caches (or any dtype: decoded by .double()); kd / vd: (B, Hk) descales or None = 1."""
    q = q.double().cpu()
    k8, v8 = k8.cpu().double(), v8.cpu().double()                                # the exact decode
    bt = None if block_table is None else block_table.cpu()
    B, Nq, H, D = q.shape
    Hk = k8.shape[2]
    G = H // Hk
    kd = torch.ones(B, Hk, dtype=torch.float64) if kd is None else kd.double().cpu()
    vd = torch.ones(B, Hk, dtype=torch.float64) if vd is None else vd.double().cpu()
    out = torch.zeros(B, Nq, H, D, dtype=torch.float64)
    lse = torch.full((B, H, Nq), math.inf, dtype=torch.float64)
    for b in range(B):
        n = int(lens[b])
        if n == 0:
            continue
        k = (gather_cache(k8, bt, b, n) * kd[b].view(1, Hk, 1)).repeat_interleave(G, dim=1)       # (n, H, D); the descale of the SEQUENCE, paged or not
        v = (gather_cache(v8, bt, b, n) * vd[b].view(1, Hk, 1)).repeat_interleave(G, dim=1)
        s = torch.einsum("qhd,khd->hqk", q[b], k) * scale
        if causal:
            i = torch.arange(Nq).view(Nq, 1)
            j = torch.arange(n).view(1, n)
            s = s.masked_fill(j > i + (n - Nq), -math.inf)
        l = torch.logsumexp(s, dim=-1)
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


def randn(gen, *shape, dtype=torch.float32, std=0.5):
    return (torch.randn(*shape, generator=gen, dtype=torch.float32) * std).to(dtype)


def uniform(gen, lo, hi, *shape):
    return lo + (hi - lo) * torch.rand(*shape, generator=gen, dtype=torch.float32)


def quantise(x, d):
    """What the append computes, on the CPU: x (B, n, Hk, D) any float dtype, d (B, Hk) float32 -> e4m3."""
    return (x.float() / d.view(d.shape[0], 1, d.shape[1], 1)).clamp(-448.0, 448.0).to(E4M3)


def make_cache(gen, B, cap, Hk, D, klo=0.002, khi=0.02, vlo=0.002, vhi=0.02):
    """A std-0.5 K and V quantised with per-(b, hk) descales: (k8, v8, kd, vd)."""
    kd, vd = uniform(gen, klo, khi, B, Hk), uniform(gen, vlo, vhi, B, Hk)
    return quantise(randn(gen, B, cap, Hk, D), kd), quantise(randn(gen, B, cap, Hk, D), vd), kd, vd


def fill_tails(k8, v8, lens, byte=NAN_BYTE):
    """Everything behind each length becomes the NaN code."""
    for b in range(k8.shape[0]):
        k8.view(torch.uint8)[b, int(lens[b]):] = byte
        v8.view(torch.uint8)[b, int(lens[b]):] = byte


def make_paged(gen, k8, v8, page, spare=3):
    """Scatter a contiguous (B, cap, Hk, D) cache into pages through a seeded shuffled block table; no page is shared; the `spare` pages hold NaN codes."""
    B, cap, Hk, D = k8.shape
    mb = cap // page
    nb = B * mb + spare
    perm = torch.randperm(nb, generator=gen)[: B * mb].view(B, mb)
    kp = torch.full((nb, page, Hk, D), NAN_BYTE, dtype=torch.uint8)
    vp = torch.full((nb, page, Hk, D), NAN_BYTE, dtype=torch.uint8)
    for b in range(B):
        for i in range(mb):
            kp[perm[b, i]] = k8.view(torch.uint8)[b, i * page:(i + 1) * page]
            vp[perm[b, i]] = v8.view(torch.uint8)[b, i * page:(i + 1) * page]
    return kp.view(E4M3), vp.view(E4M3), perm.to(torch.int32)


def run(q, k8, v8, lens, kd=None, vd=None, bt=None, k=None, v=None, causal=False, splits=0, scale=None):
    d = lambda t: None if t is None else t.to(DEV)
    out, lse = tfa.flash_attn_with_kvcache(d(q), d(k8), d(v8), d(k), d(v), cache_seqlens=d(lens), block_table=d(bt), softmax_scale=scale, causal=causal,
                                           num_splits=splits, return_softmax_lse=True, k_descale=d(kd), v_descale=d(vd))
    torch.cuda.synchronize()
    return out, lse


# ---- 1. contiguous cache, ragged lengths -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [64, 128, 48, 112])
def test_contiguous_ragged_lengths(dtype, D):
    gen = torch.Generator().manual_seed(100 + D)
    B, H, Hk, cap = 5, 8, 8, 1024
    lens = torch.tensor([512, 700, 1, 0, 1024], dtype=torch.int32)               # a multiple of 64, a non-multiple, 1, 0, the capacity
    q = randn(gen, B, 1, H, D, dtype=dtype, std=1.0)
    k8, v8, kd, vd = make_cache(gen, B, cap, Hk, D)
    fill_tails(k8, v8, lens)
    scale = 1.0 / math.sqrt(D)
    ref = reference(q, k8, v8, kd, vd, lens, None, scale, False)
    for splits in (1, 4):
        out, lse = run(q, k8, v8, lens, kd, vd, splits=splits)
        assert out.dtype == dtype
        assert_matches(out, lse, *ref, what=f"contiguous {dtype} D{D} splits{splits}")
        assert (out[3] == 0).all() and torch.isinf(lse[3]).all() and (lse[3] > 0).all()      # the empty sequence


# ---- 2. paged cache, NaN codes in the spare pages and behind every length ------------------------------------------------------------------
@pytest.mark.parametrize("page", [64, 256])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_paged_cache_with_nan_codes_behind_the_lengths(page, dtype):
    gen = torch.Generator().manual_seed(31 + page)
    B, H, Hk, D, cap = 4, 8, 4, 128, 1024
    lens = torch.tensor([1024, 333, 640, 65], dtype=torch.int32)
    q = randn(gen, B, 1, H, D, dtype=dtype, std=1.0)
    k8, v8, kd, vd = make_cache(gen, B, cap, Hk, D)
    fill_tails(k8, v8, lens)
    kp, vp, bt = make_paged(gen, k8, v8, page)
    assert len(set(bt.flatten().tolist())) == bt.numel()                          # no page shared
    scale = 1.0 / math.sqrt(D)
    ref = reference(q, kp, vp, kd, vd, lens, bt, scale, False)
    assert torch.equal(ref[0], reference(q, k8, v8, kd, vd, lens, None, scale, False)[0])
    for splits in (1, 4):
        out, lse = run(q, kp, vp, lens, kd, vd, bt, splits=splits)
        assert not torch.isnan(out).any() and not torch.isnan(lse).any()
        assert_matches(out, lse, *ref, what=f"paged{page} {dtype} splits{splits}")
        out_c, lse_c = run(q, k8, v8, lens, kd, vd, None, splits=splits)
        assert torch.equal(out, out_c) and torch.equal(lse, lse_c), "paged and contiguous results differ in bits"


# ---- 3. GQA packed, MQA, MHA; several rows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Hk", [(32, 8), (8, 1), (8, 8)])
@pytest.mark.parametrize("paged", [False, True])
def test_gqa_mqa_mha_decode(H, Hk, paged):
    gen = torch.Generator().manual_seed(50 + H + Hk)
    dtype, B, D, cap = torch.float16, 3, 128, 2048
    lens = torch.tensor([2048, 777, 64], dtype=torch.int32)
    q = randn(gen, B, 1, H, D, dtype=dtype, std=1.0)
    k8, v8, kd, vd = make_cache(gen, B, cap, Hk, D)
    fill_tails(k8, v8, lens)
    scale = 1.0 / math.sqrt(D)
    ref = reference(q, k8, v8, kd, vd, lens, None, scale, True)                   # one row: causal or not is the same
    bt = None
    if paged:
        k8, v8, bt = make_paged(gen, k8, v8, 128)
    for causal in (False, True):
        for splits in (1, 4):
            out, lse = run(q, k8, v8, lens, kd, vd, bt, causal=causal, splits=splits)
            assert_matches(out, lse, *ref, what=f"H{H} Hk{Hk} paged={paged} causal={causal} splits{splits}")


@pytest.mark.parametrize("Nq,causal", [(5, True), (300, True), (300, False)])
@pytest.mark.parametrize("paged", [False, True])
def test_several_rows(Nq, causal, paged):
    gen = torch.Generator().manual_seed(60 + Nq)
    dtype, B, H, Hk, D, cap = torch.bfloat16, 4, 8, 2, 64, 1024
    lens = torch.tensor([1000, 3, Nq, 513], dtype=torch.int32)                   # one sequence shorter than Nq: causal, its first rows see nothing
    q = randn(gen, B, Nq, H, D, dtype=dtype, std=1.0)
    k8, v8, kd, vd = make_cache(gen, B, cap, Hk, D)
    fill_tails(k8, v8, lens)
    scale = 1.0 / math.sqrt(D)
    ref = reference(q, k8, v8, kd, vd, lens, None, scale, causal)
    if causal:
        assert torch.isinf(ref[1][1, :, : Nq - 3]).all() and torch.isfinite(ref[1][1, :, Nq - 3:]).all()
    bt = None
    if paged:
        k8, v8, bt = make_paged(gen, k8, v8, 64)
    for splits in (1, 3):
        out, lse = run(q, k8, v8, lens, kd, vd, bt, causal=causal, splits=splits)
        assert_matches(out, lse, *ref, what=f"Nq{Nq} causal={causal} paged={paged} splits{splits}")


# ---- 4. bite for the descales ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splits", [1, 2])
def test_descales_bite(splits):
    """On the same bytes, the reference with all descales 1, with only one of them 1, and with k and v descales swapped each miss the true reference by more than
    10x the bar: a kernel that ignored or confused a scale cannot pass.  (Short sequences and two ranges, so that out is O(1) and the scales differ by 2x and more.)"""
    gen = torch.Generator().manual_seed(44)
    dtype, B, H, Hk, D, cap = torch.bfloat16, 4, 8, 4, 128, 256
    lens = torch.tensor([3, 8, 130, 256], dtype=torch.int32)
    q = randn(gen, B, 1, H, D, dtype=dtype, std=1.0)
    k8, v8, kd, vd = make_cache(gen, B, cap, Hk, D, klo=0.002, khi=0.006, vlo=0.012, vhi=0.02)
    scale = 1.0 / math.sqrt(D)
    ref = reference(q, k8, v8, kd, vd, lens, None, scale, False)
    one = torch.ones_like(kd)
    for name, wk, wv in (("no descale", one, one), ("no k_descale", one, vd), ("no v_descale", kd, one), ("swapped", vd, kd)):
        wrong = reference(q, k8, v8, wk, wv, lens, None, scale, False)
        miss = (wrong[0] - ref[0]).abs().max().item()
        print(f"{name}: the reference misses by {miss:.3e}")
        assert miss > 10 * OUT_BAR, name
    out, lse = run(q, k8, v8, lens, kd, vd, splits=splits)
    assert_matches(out, lse, *ref, what=f"descales bite splits{splits}")
    # per-tensor scales as expanded (stride 0) tensors, and descales with transposed strides
    kd1, vd1 = torch.tensor([[0.004]]), torch.tensor([[0.015]])
    ref1 = reference(q, k8, v8, kd1.expand(B, Hk), vd1.expand(B, Hk), lens, None, scale, False)
    out, lse = tfa.flash_attn_with_kvcache(q.to(DEV), k8.to(DEV), v8.to(DEV), cache_seqlens=lens.to(DEV), num_splits=splits, return_softmax_lse=True,
                                           k_descale=kd1.to(DEV).expand(B, Hk), v_descale=vd1.to(DEV).expand(B, Hk))
    assert_matches(out, lse, *ref1, what=f"expanded per-tensor descales splits{splits}")
    kdt, vdt = kd.t().contiguous().to(DEV).t(), vd.t().contiguous().to(DEV).t()
    assert kdt.stride() == (1, B)
    out, lse = tfa.flash_attn_with_kvcache(q.to(DEV), k8.to(DEV), v8.to(DEV), cache_seqlens=lens.to(DEV), num_splits=splits, return_softmax_lse=True,
                                           k_descale=kdt, v_descale=vdt)
    assert_matches(out, lse, *ref, what=f"transposed descales splits{splits}")


# ---- 5. bite for the decode: every finite code ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("descale", [1.0, 0.125])
def test_every_finite_code_decodes_exactly(dtype, descale):
    """Two sequences of ONE key each; the key row of sequence b holds the codes 128 b .. 128 b + 127 in K, and the same codes in another order in V (the two NaN
    codes replaced by 0x00): all 254 finite codes, at every byte position of a chunk.  128 one-hot query rows: row i's only score is dec(k[i]) * descale, which is its
    LSE, and P = 1 exactly, so out = dec(v) * descale — every code pinned, K through the LSE and V through out.  e4m3 -> bf16 / f16 is exact and the descales are powers
    of two, so out must equal the reference within the output format's rounding: 2^-8 relative (bf16 keeps 8 significant bits), not the 1e-2 bar."""
    codes = torch.arange(256, dtype=torch.uint8)
    finite = ~torch.isnan(codes.view(E4M3).float())
    assert int(finite.sum()) == 254
    codes[~finite] = 0
    B, D = 2, 128
    k8 = codes.view(B, 1, 1, D).clone().view(E4M3)
    v8 = codes.view(B, 1, 1, D).flip(-1).roll(37, -1).clone().view(E4M3)
    assert len(set(k8.view(torch.uint8).flatten().tolist())) == 254 == len(set(v8.view(torch.uint8).flatten().tolist()))     # every finite code, +0 and -0 among them
    q = torch.eye(D, dtype=dtype).view(1, D, 1, D).repeat(B, 1, 1, 1).contiguous()
    lens = torch.ones(B, dtype=torch.int32)
    kd = torch.full((B, 1), descale)
    ref_out, ref_lse = reference(q, k8, v8, kd, kd, lens, None, 1.0, False)
    assert torch.equal(ref_lse[:, 0], k8.double().view(B, D) * descale)
    assert torch.equal(ref_out[:, 0, 0], v8.double().view(B, D) * descale)
    for paged in (False, True):
        kk, vv, bt = k8, v8, None
        if paged:
            kk = torch.full((3, 64, 1, D), NAN_BYTE, dtype=torch.uint8)
            vv = torch.full((3, 64, 1, D), NAN_BYTE, dtype=torch.uint8)
            bt = torch.tensor([[2], [0]], dtype=torch.int32)
            for b in range(B):
                kk[int(bt[b, 0]), 0] = k8.view(torch.uint8)[b, 0]
                vv[int(bt[b, 0]), 0] = v8.view(torch.uint8)[b, 0]
            kk, vv = kk.view(E4M3), vv.view(E4M3)
        out, lse = run(q, kk, vv, lens, kd, kd, bt, splits=1, scale=1.0)
        assert_matches(out, lse, ref_out, ref_lse, what=f"all codes {dtype} descale {descale} paged={paged}")
        o = out.double().cpu()
        excess = ((o - ref_out).abs() - ref_out.abs() * 2.0 ** -8).max().item()
        print(f"all codes {dtype} descale {descale} paged={paged}: max excess over 2^-8 relative = {excess:.3e}")
        assert excess <= 0.0
        l_err = ((lse.double().cpu() - ref_lse).abs() - ref_lse.abs() * 2.0 ** -20).max().item()
        assert l_err <= 1e-7, f"a K code is decoded to another value: {l_err}"


# ---- 6. bit identity with the 16-bit path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("H,Hk,Nq,causal", [(32, 8, 1, False), (8, 2, 5, True), (8, 8, 1, False)])
def test_bit_identity_with_the_16_bit_path(dtype, paged, H, Hk, Nq, causal):
    """Without descales — None, and all-ones tensors — out and lse equal BIT FOR BIT what the 16-bit path returns for the caches converted to q's dtype, for the same
    num_splits: the decode is exact and the arithmetic behind it is the same (no fp8 MFMA, no quantised Q or P)."""
    gen = torch.Generator().manual_seed(600 + H + Nq)
    B, D, cap = 3, 128, 2048
    lens = torch.tensor([2048, 777, 65], dtype=torch.int32)
    q = randn(gen, B, Nq, H, D, dtype=dtype, std=1.0)
    one = torch.ones(B, Hk)
    k8, v8 = quantise(randn(gen, B, cap, Hk, D), one), quantise(randn(gen, B, cap, Hk, D), one)      # values of the size the 16-bit tests use, on the e4m3 grid
    bt = None
    if paged:
        k8, v8, bt = make_paged(gen, k8, v8, 128)
        k8.view(torch.uint8)[k8.view(torch.uint8) == NAN_BYTE] = 0                 # (the 16-bit twin of a NaN page would be NaN as well: same bits, but keep it plain)
        v8.view(torch.uint8)[v8.view(torch.uint8) == NAN_BYTE] = 0
    k16, v16 = k8.to(dtype), v8.to(dtype)
    assert torch.equal(k16.float(), k8.float())                                    # exact
    d = lambda t: None if t is None else t.to(DEV)
    for splits in (1, 4):
        want = tfa.flash_attn_with_kvcache(d(q), d(k16), d(v16), cache_seqlens=d(lens), block_table=d(bt), causal=causal, num_splits=splits, return_softmax_lse=True)
        for kd, vd in ((None, None), (one, one), (one, None)):
            got = run(q, k8, v8, lens, kd, vd, bt, causal=causal, splits=splits)
            assert torch.equal(got[0].view(torch.int16), want[0].view(torch.int16)), f"out differs in bits (splits {splits}, descales {'ones' if kd is not None else None})"
            assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), f"lse differs in bits (splits {splits})"
    assert_matches(*got, *reference(q, k8, v8, None, None, lens, bt, 1.0 / math.sqrt(D), causal), what=f"bit identity {dtype} paged={paged} H{H} Nq{Nq}")


# ---- 7. append -------------------------------------------------------------------------------------------------------------------------------
CANARY = 0x7B


def carve(shape, pad=4096):
    """An e4m3 cache carved out of a larger device allocation with a canary byte on both sides: (the whole uint8 buffer, the carved cache)."""
    numel = math.prod(shape)
    whole = torch.full((pad + numel + pad,), CANARY, dtype=torch.uint8, device=DEV)
    return whole, whole[pad:pad + numel].view(E4M3).view(shape)


def special_rows(dtype, d, D):
    """New rows whose quotients x / d hit the clamp, the ties and the subnormal range of e4m3 (d: this row's descale, a float)."""
    targets = [448.0, 449.0, 464.0, 465.0, 480.0, 1000.0, 1e6, -448.0, -464.0, -1e5, 0.0, -0.0, 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, 5 * 2.0 ** -10, 2.0 ** -11,
               0.0146, 0.0156, 2.0 ** -6, 1.0625, 1.1875, 1.3125, 17.0, 18.0, 19.0, 22.0, 26.0, 208.0, 240.0, 432.0, 447.0, float("inf"), float("-inf")]
    x = torch.tensor(targets, dtype=torch.float32) * d
    return torch.cat([x, x.flip(0)])[:D].to(dtype) if 2 * len(targets) >= D else torch.cat([x] * (D // len(targets) + 1))[:D].to(dtype)


@pytest.mark.parametrize("n_new", [1, 3])
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("pow2", [True, False])
def test_append_quantises_in_place(n_new, paged, dtype, pow2):
    gen = torch.Generator().manual_seed(70 + n_new)
    B, H, Hk, D, cap, page = 5, 8, 2, 64, 512, 128
    # room for all rows, the last row only just, one row too many, full, beyond the capacity (a bad length: nothing written, everything attended)
    lens = torch.tensor([100, cap - n_new, cap - 1, cap, cap + 7], dtype=torch.int32)
    q = randn(gen, B, n_new, H, D, dtype=dtype, std=1.0)
    k8, v8, kd, vd = make_cache(gen, B, cap, Hk, D)
    if pow2:
        kd = 2.0 ** torch.randint(-9, -5, (B, Hk), generator=gen).float()
        vd = 2.0 ** torch.randint(-9, -5, (B, Hk), generator=gen).float()
    kn, vn = randn(gen, B, n_new, Hk, D, dtype=dtype), randn(gen, B, n_new, Hk, D, dtype=dtype)
    for b in range(B):                                                            # the clamp, the ties and the subnormals, in one head of K and the other of V
        kn[b, 0, 0] = special_rows(dtype, float(kd[b, 0]), D)
        vn[b, n_new - 1, 1] = special_rows(dtype, float(vd[b, 1]), D)
    kn[0, 0, 1, 5] = float("nan")                                                  # a NaN input stays NaN (sequence 0 has room for it)
    kq, vq = quantise(kn, kd), quantise(vn, vd)
    assert (kq.float().abs() == 448).any() and ((kq.float() != 0) & (kq.float().abs() < 2.0 ** -6)).any()      # the inputs reach the clamp and the subnormals
    bt = None
    if paged:
        k8, v8, bt = make_paged(gen, k8, v8, page)
        k8.view(torch.uint8)[k8.view(torch.uint8) == NAN_BYTE] = 0x38            # (spare pages: a finite code, so that NaN below means the appended NaN)
        v8.view(torch.uint8)[v8.view(torch.uint8) == NAN_BYTE] = 0x38
    # the expected caches, on the CPU, and the positions written
    ke, ve = k8.clone(), v8.clone()
    written = torch.zeros(k8.shape[:2], dtype=torch.bool)
    for b in range(B):
        for t in range(n_new):
            pos = int(lens[b]) + t
            if pos >= cap:
                continue
            at = (int(bt[b, pos // page]), pos % page) if paged else (b, pos)
            ke.view(torch.uint8)[at] = kq.view(torch.uint8)[b, t]
            ve.view(torch.uint8)[at] = vq.view(torch.uint8)[b, t]
            written[at] = True
    assert torch.isnan(ke.float()).sum() == 1
    after = torch.clamp(lens + n_new, max=cap)
    scale = 1.0 / math.sqrt(D)
    ke_ref = ke.clone()
    ke_ref.view(torch.uint8)[torch.isnan(ke.float())] = 0                          # the reference attends the appended NaN as 0 ...
    k_whole, k_dev = carve(k8.shape)
    v_whole, v_dev = carve(v8.shape)
    lens_dev = lens.to(DEV)
    pad = (k_whole.numel() - k8.numel()) // 2
    for splits in (1, 2):
        k_dev.view(torch.uint8).copy_(k8.view(torch.uint8))
        v_dev.view(torch.uint8).copy_(v8.view(torch.uint8))
        out, lse = tfa.flash_attn_with_kvcache(q.to(DEV), k_dev, v_dev, kn.to(DEV), vn.to(DEV), cache_seqlens=lens_dev, block_table=None if bt is None else bt.to(DEV),
                                               causal=True, num_splits=splits, return_softmax_lse=True, k_descale=kd.to(DEV), v_descale=vd.to(DEV))
        torch.cuda.synchronize()
        assert torch.equal(lens_dev.cpu(), lens), "cache_seqlens was modified"
        for whole, dev, want, name in ((k_whole, k_dev, ke, "k"), (v_whole, v_dev, ve, "v")):
            got = dev.cpu()
            g, w = got.float(), want.float()
            assert torch.equal(torch.isnan(g), torch.isnan(w)), f"{name}_cache: NaN elsewhere than expected"
            bad = (g != w) & ~torch.isnan(w)
            assert not bad.any(), f"{name}_cache: {int(bad.sum())} appended elements differ from torch's quantisation, e.g. got {g[bad][:4].tolist()} want {w[bad][:4].tolist()}"
            assert torch.equal(got.view(torch.uint8)[~written], want.view(torch.uint8)[~written]), f"{name}_cache changed outside the appended rows"
            wb = whole.cpu()
            assert (wb[:pad] == CANARY).all() and (wb[pad + want.numel():] == CANARY).all(), f"a canary around {name}_cache was overwritten"
        # ... which the kernel cannot: compare the sequences without it (the NaN sits in sequence 0's head 1) and, for sequence 0, the heads of K/V head 0
        ref = reference(q, ke_ref, ve, kd, vd, after, bt, scale, True)
        o, l = out.clone(), lse.clone()
        G = H // Hk
        o[0, :, G:] = ref[0][0, :, G:].to(o.dtype)
        l[0, G:] = ref[1][0, G:].float()
        assert_matches(o, l, *ref, what=f"append n_new{n_new} paged={paged} {dtype} pow2={pow2} splits{splits}")


# ---- 8. a captured decode step: lengths advanced and descales overwritten in place -----------------------------------------------------------
@pytest.mark.parametrize("paged", [False, True])
def test_captured_decode_step_sees_new_lengths_and_descales(paged):
    gen = torch.Generator().manual_seed(8)
    dtype, B, H, Hk, D, cap = torch.bfloat16, 4, 8, 2, 128, 4096
    lens = torch.tensor([4000, 17, 2048, 0], dtype=torch.int32)
    k8, v8, kd, vd = make_cache(gen, B, cap, Hk, D)
    bt = None
    if paged:
        k8, v8, bt = make_paged(gen, k8, v8, 256)
    steps = [(randn(gen, B, 1, H, D, dtype=dtype, std=1.0), randn(gen, B, 1, Hk, D, dtype=dtype), randn(gen, B, 1, Hk, D, dtype=dtype)) for _ in range(4)]
    k_dev, v_dev, lens_dev, kd_dev, vd_dev = k8.to(DEV), v8.to(DEV), lens.to(DEV), kd.to(DEV), vd.to(DEV)
    bt_dev = None if bt is None else bt.to(DEV)
    q_s, k_s, v_s = (t.to(DEV).clone() for t in steps[0])
    call = lambda: tfa.flash_attn_with_kvcache(q_s, k_dev, v_dev, k_s, v_s, cache_seqlens=lens_dev, block_table=bt_dev, causal=True, num_splits=0,
                                               return_softmax_lse=True, k_descale=kd_dev, v_descale=vd_dev)
    call()                                                                        # one warm-up call outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_s, lse_s = call()
    scale = 1.0 / math.sqrt(D)
    # the CPU mirror starts from what the device holds now (the warm-up and the capture did not run the captured work twice on other data: both appended step 0 at lens)
    kc_cpu, vc_cpu, cur = k_dev.cpu(), v_dev.cpu(), lens.clone()
    for r in range(1, 4):
        qr, kr, vr = steps[r]
        q_s.copy_(qr.to(DEV))
        k_s.copy_(kr.to(DEV))
        v_s.copy_(vr.to(DEV))
        kd = kd * (1.5 if r == 2 else 1.0)                                        # the descales change under the captured graph, in place
        vd = vd * (0.5 if r == 2 else 1.0)
        kd_dev.copy_(kd.to(DEV))
        vd_dev.copy_(vd.to(DEV))
        g.replay()
        torch.cuda.synchronize()
        kq, vq = quantise(kr, kd), quantise(vr, vd)
        for b in range(B):                                                        # the CPU mirror of the append
            pos = int(cur[b])
            at = (int(bt[b, pos // 256]), pos % 256) if paged else (b, pos)
            kc_cpu.view(torch.uint8)[at] = kq.view(torch.uint8)[b, 0]
            vc_cpu.view(torch.uint8)[at] = vq.view(torch.uint8)[b, 0]
        ref = reference(qr, kc_cpu, vc_cpu, kd, vd, cur + 1, bt, scale, True)
        if r == 2:
            stale = reference(qr, kc_cpu, vc_cpu, kd / 1.5, vd / 0.5, cur + 1, bt, scale, True)
            assert (stale[0] - ref[0]).abs().max().item() > 10 * OUT_BAR         # the captured values would miss
        assert_matches(out_s, lse_s, *ref, what=f"replay {r} paged={paged}")
        lens_dev.add_(1)                                                          # the caller advances the lengths, in place on the device
        cur = cur + 1
    torch.cuda.synchronize()


# ---- 9. seeded random sweep ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(40))
def test_seeded_sweep(seed):
    gen = torch.Generator().manual_seed(9800 + seed)
    pick = lambda xs: xs[int(torch.randint(len(xs), (1,), generator=gen))]
    dtype = pick([torch.bfloat16, torch.float16])
    B = pick([1, 2, 3, 5])
    Hk = pick([1, 2, 4])
    H = Hk * pick([1, 2, 4, 8])
    D = pick([16, 32, 48, 64, 80, 96, 112, 128])
    paged = pick([False, True])
    page = pick([64, 128, 192, 256])
    cap = page * pick([2, 3, 5]) if paged else pick([64, 100, 777, 1024, 1500])
    Nq = pick([1, 1, 1, 2, 5, 17, 130])
    causal = pick([False, True])
    splits = pick([0, 1, 2, 3, 8])
    n_new = pick([0, 0, 1, 2]) if Nq <= 17 else 0
    descales = pick(["both", "both", "k", "v", "none"])
    lens = torch.randint(0, cap + 1 - n_new, (B,), generator=gen).to(torch.int32)
    if seed % 5 == 0:
        lens[0] = cap - n_new
    if seed % 7 == 0:
        lens[-1] = 0
    q = randn(gen, B, Nq, H, D, dtype=dtype, std=1.0)
    k8, v8, kd, vd = make_cache(gen, B, cap, Hk, D)
    if descales in ("v", "none"):
        kd = None
        k8 = quantise(randn(gen, B, cap, Hk, D), torch.ones(B, Hk))
    if descales in ("k", "none"):
        vd = None
        v8 = quantise(randn(gen, B, cap, Hk, D), torch.ones(B, Hk))
    fill_tails(k8, v8, lens)                                                      # NaN codes behind every length (the appended rows overwrite theirs)
    kn = vn = None
    ke, ve = k8.clone(), v8.clone()
    if n_new:
        kn, vn = randn(gen, B, n_new, Hk, D, dtype=dtype), randn(gen, B, n_new, Hk, D, dtype=dtype)
        one = torch.ones(B, Hk)
        kq, vq = quantise(kn, one if kd is None else kd), quantise(vn, one if vd is None else vd)
        for b in range(B):
            n = int(lens[b])
            ke.view(torch.uint8)[b, n:n + n_new] = kq.view(torch.uint8)[b]
            ve.view(torch.uint8)[b, n:n + n_new] = vq.view(torch.uint8)[b]
    scale = pick([1.0 / math.sqrt(D), 0.05])
    ref = reference(q, ke, ve, kd, vd, lens + n_new, None, scale, causal)
    bt = None
    if paged:
        k8, v8, bt = make_paged(gen, k8, v8, page)
    out, lse = run(q, k8, v8, lens, kd, vd, bt, kn, vn, causal=causal, splits=splits, scale=scale)
    assert_matches(out, lse, *ref, what=f"seed{seed} {dtype} B{B} H{H} Hk{Hk} D{D} paged={paged} page{page} cap{cap} Nq{Nq} n_new{n_new} causal={causal} "
                                        f"splits{splits} descales={descales}")
