"""GPU tests of ``flash_attn_with_kvcache`` (tfa_fwd_kvcache, tfa_kvcache_append): device-side lengths, contiguous and paged caches, split counts, GQA / MQA
decode, several causal rows, the in-place append with its capacity clamp, a captured decode step, and a seeded sweep.

The reference is written here: for each sequence the keys [0, len_b) are gathered from the cache through the block table, and the scores, the causal mask at
shift_b = len_b - Nq, the logsumexp and P @ v are computed in fp64 on the CPU.  Bars (include/tfa.h): 16-bit out |d| <= 1e-2; LSE |d| <= 1e-4 * max(1, |ref|)
and +inf exactly on rows that see no key.  Every case compares every output element."""
import math

import pytest
import torch

import tiny_flash_attention_amd as tfa

pytestmark = pytest.mark.gpu

OUT_BAR = 1e-2
LSE_BAR = 1e-4
DEV = "cuda:0"


def gather_cache(cache, block_table, b, n):
    """Keys [0, n) of sequence b as (n, Hk, D): rows of the contiguous cache, or of its pages in block-table order."""
    if block_table is None:
        return cache[b, :n]
    page = cache.shape[1]
    pages = [cache[int(block_table[b, i])] for i in range((n + page - 1) // page)]
    return torch.cat(pages, 0)[:n] if pages else cache[0, :0]


def reference(q, k_cache, v_cache, lens, block_table, scale, causal):
    """fp64 attention of every sequence over its own keys: out (B, Nq, H, D), lse (B, H, Nq); rows that see no key: out = 0, lse = +inf."""
    q, k_cache, v_cache = q.double().cpu(), k_cache.double().cpu(), v_cache.double().cpu()
    bt = None if block_table is None else block_table.cpu()
    B, Nq, H, D = q.shape
    Hk = k_cache.shape[2]
    G = H // Hk
    out = torch.zeros(B, Nq, H, D, dtype=torch.float64)
    lse = torch.full((B, H, Nq), math.inf, dtype=torch.float64)
    for b in range(B):
        n = int(lens[b])
        if n == 0:
            continue
        k = gather_cache(k_cache, bt, b, n).repeat_interleave(G, dim=1)          # (n, H, D)
        v = gather_cache(v_cache, bt, b, n).repeat_interleave(G, dim=1)
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


def make_paged(gen, kc, vc, page, spare=3):
    """Scatter a contiguous (B, cap, Hk, D) cache into pages through a seeded shuffled block table; no page is shared; `spare` unused pages hold garbage."""
    B, cap, Hk, D = kc.shape
    mb = cap // page
    nb = B * mb + spare
    perm = torch.randperm(nb, generator=gen)[: B * mb].view(B, mb)
    kp = randn(gen, nb, page, Hk, D, dtype=kc.dtype, std=3.0)
    vp = randn(gen, nb, page, Hk, D, dtype=kc.dtype, std=3.0)
    for b in range(B):
        for i in range(mb):
            kp[perm[b, i]] = kc[b, i * page:(i + 1) * page]
            vp[perm[b, i]] = vc[b, i * page:(i + 1) * page]
    return kp, vp, perm.to(torch.int32)


def run(q, kc, vc, lens, bt=None, k=None, v=None, causal=False, splits=0, scale=None):
    d = lambda t: None if t is None else t.to(DEV)
    out, lse = tfa.flash_attn_with_kvcache(d(q), d(kc), d(vc), d(k), d(v), cache_seqlens=d(lens), block_table=d(bt), softmax_scale=scale, causal=causal,
                                           num_splits=splits, return_softmax_lse=True)
    torch.cuda.synchronize()
    return out, lse


# ---- 1. contiguous cache, ragged lengths -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [64, 128, 40, 104])
def test_contiguous_ragged_lengths(dtype, D):
    gen = torch.Generator().manual_seed(100 + D)
    B, H, Hk, cap = 5, 8, 8, 1024
    lens = torch.tensor([512, 700, 1, 0, 1024], dtype=torch.int32)               # a multiple of 64, a non-multiple, 1, 0, the capacity
    q = randn(gen, B, 1, H, D, dtype=dtype, std=1.0)
    kc, vc = randn(gen, B, cap, Hk, D, dtype=dtype), randn(gen, B, cap, Hk, D, dtype=dtype)
    scale = 1.0 / math.sqrt(D)
    ref = reference(q, kc, vc, lens, None, scale, False)
    for splits in (1, 4):
        out, lse = run(q, kc, vc, lens, splits=splits)
        assert_matches(out, lse, *ref, what=f"contiguous {dtype} D{D} splits{splits}")
        assert (out[3] == 0).all() and torch.isinf(lse[3]).all() and (lse[3] > 0).all()      # the empty sequence


# ---- 2. bite for the lengths -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("garbage", ["nan", "finite"])
def test_what_lies_behind_the_length_is_never_read(garbage, paged):
    gen = torch.Generator().manual_seed(7)
    dtype, B, H, Hk, D, cap = torch.bfloat16, 4, 8, 2, 128, 1024
    lens = torch.tensor([300, 64, 1000, 0], dtype=torch.int32)
    q = randn(gen, B, 1, H, D, dtype=dtype, std=1.0)
    kc, vc = randn(gen, B, cap, Hk, D, dtype=dtype), randn(gen, B, cap, Hk, D, dtype=dtype)
    for b in range(B):
        n = int(lens[b])
        if garbage == "nan":
            kc[b, n:] = float("nan")
            vc[b, n:] = float("nan")
        else:
            kc[b, n:] = randn(gen, cap - n, Hk, D, dtype=dtype, std=4.0)
            vc[b, n:] = 100.0
    scale = 1.0 / math.sqrt(D)
    ref = reference(q, kc, vc, lens, None, scale, False)
    if garbage == "finite":
        # the inputs bite: a kernel that ignored the lengths would compute this, which misses the bar by more than 10x
        wrong, _ = reference(q, kc, vc, torch.full((B,), cap, dtype=torch.int32), None, scale, False)
        miss = (wrong - ref[0]).abs().max().item()
        print(f"full-capacity reference misses by {miss:.3e}")
        assert miss >= 10 * OUT_BAR
    bt = None
    if paged:
        kc, vc, bt = make_paged(gen, kc, vc, 128)
        if garbage == "nan":                                                     # the spare pages too
            used = set(bt.flatten().tolist())
            for pg in range(kc.shape[0]):
                if pg not in used:
                    kc[pg] = float("nan")
                    vc[pg] = float("nan")
    for splits in (1, 3):
        out, lse = run(q, kc, vc, lens, bt, splits=splits)
        assert not torch.isnan(out).any() and not torch.isnan(lse).any()
        assert_matches(out, lse, *ref, what=f"garbage={garbage} paged={paged} splits{splits}")


# ---- 3. paged cache --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page", [64, 128, 256])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_paged_cache_matches_reference_and_contiguous_bits(page, dtype):
    gen = torch.Generator().manual_seed(31 + page)
    B, H, Hk, D, cap = 4, 8, 4, 128, 1024
    lens = torch.tensor([1024, 333, 640, 65], dtype=torch.int32)
    q = randn(gen, B, 1, H, D, dtype=dtype, std=1.0)
    kc, vc = randn(gen, B, cap, Hk, D, dtype=dtype), randn(gen, B, cap, Hk, D, dtype=dtype)
    kp, vp, bt = make_paged(gen, kc, vc, page)
    assert len(set(bt.flatten().tolist())) == bt.numel()                          # no page shared
    scale = 1.0 / math.sqrt(D)
    ref = reference(q, kp, vp, lens, bt, scale, False)
    ref_c = reference(q, kc, vc, lens, None, scale, False)
    assert torch.equal(ref[0], ref_c[0])                                          # the same keys either way
    identity = torch.arange(B * (cap // page), dtype=torch.int32).view(B, -1)
    wrong, _ = reference(q, kp, vp, lens, identity, scale, False)                 # a kernel that ignored the table would compute this
    miss = (wrong - ref[0]).abs().max().item()
    print(f"identity-table reference misses by {miss:.3e}")
    assert miss >= 10 * OUT_BAR
    for splits in (1, 4):
        out, lse = run(q, kp, vp, lens, bt, splits=splits)
        assert_matches(out, lse, *ref, what=f"paged{page} {dtype} splits{splits}")
        out_c, lse_c = run(q, kc, vc, lens, None, splits=splits)
        assert torch.equal(out, out_c) and torch.equal(lse, lse_c), "paged and contiguous results differ in bits"


# ---- 4. splits -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged", [False, True])
def test_split_counts_agree_and_runs_are_bit_equal(paged):
    gen = torch.Generator().manual_seed(4)
    dtype, B, H, Hk, D, cap = torch.bfloat16, 3, 8, 8, 64, 8192
    lens = torch.tensor([8192, 5000, 130], dtype=torch.int32)
    q = randn(gen, B, 1, H, D, dtype=dtype, std=1.0)
    kc, vc = randn(gen, B, cap, Hk, D, dtype=dtype), randn(gen, B, cap, Hk, D, dtype=dtype)
    scale = 1.0 / math.sqrt(D)
    ref = reference(q, kc, vc, lens, None, scale, False)
    bt = None
    if paged:
        kc, vc, bt = make_paged(gen, kc, vc, 256)
    for splits in (1, 2, 8, 0):
        out, lse = run(q, kc, vc, lens, bt, splits=splits)
        assert_matches(out, lse, *ref, what=f"splits={splits} paged={paged}")
        out2, lse2 = run(q, kc, vc, lens, bt, splits=splits)
        assert torch.equal(out, out2) and torch.equal(lse, lse2), "two runs of the same call differ"


# ---- 5. GQA and MQA decode -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Hk", [(16, 2), (8, 1), (32, 4)])
@pytest.mark.parametrize("paged", [False, True])
def test_gqa_mqa_decode(H, Hk, paged):
    gen = torch.Generator().manual_seed(50 + H)
    dtype, B, D, cap = torch.float16, 3, 128, 2048
    lens = torch.tensor([2048, 777, 64], dtype=torch.int32)
    q = randn(gen, B, 1, H, D, dtype=dtype, std=1.0)
    kc, vc = randn(gen, B, cap, Hk, D, dtype=dtype), randn(gen, B, cap, Hk, D, dtype=dtype)
    scale = 1.0 / math.sqrt(D)
    ref = reference(q, kc, vc, lens, None, scale, True)                           # one row: causal or not is the same
    bt = None
    if paged:
        kc, vc, bt = make_paged(gen, kc, vc, 128)
    for causal in (False, True):
        for splits in (1, 4):
            out, lse = run(q, kc, vc, lens, bt, causal=causal, splits=splits)
            assert_matches(out, lse, *ref, what=f"H{H} Hk{Hk} paged={paged} causal={causal} splits{splits}")


# ---- 6. speculative / chunked decode ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nq", [5, 17])
@pytest.mark.parametrize("paged", [False, True])
def test_several_causal_rows_bottom_right_per_sequence(Nq, paged):
    gen = torch.Generator().manual_seed(60 + Nq)
    dtype, B, H, Hk, D, cap = torch.bfloat16, 4, 8, 2, 64, 1024
    lens = torch.tensor([1000, 3, Nq, 513], dtype=torch.int32)                   # one sequence shorter than Nq: its first rows see nothing
    q = randn(gen, B, Nq, H, D, dtype=dtype, std=1.0)
    kc, vc = randn(gen, B, cap, Hk, D, dtype=dtype), randn(gen, B, cap, Hk, D, dtype=dtype)
    scale = 1.0 / math.sqrt(D)
    ref = reference(q, kc, vc, lens, None, scale, True)
    assert torch.isinf(ref[1][1, :, : Nq - 3]).all() and torch.isfinite(ref[1][1, :, Nq - 3:]).all()
    bt = None
    if paged:
        kc, vc, bt = make_paged(gen, kc, vc, 64)
    for splits in (1, 3):
        out, lse = run(q, kc, vc, lens, bt, causal=True, splits=splits)
        assert_matches(out, lse, *ref, what=f"Nq{Nq} paged={paged} splits{splits}")
    ref_nc = reference(q, kc, vc, lens, bt, scale, False)
    out, lse = run(q, kc, vc, lens, bt, causal=False, splits=2)
    assert_matches(out, lse, *ref_nc, what=f"Nq{Nq} paged={paged} non-causal")


# ---- 7. append -------------------------------------------------------------------------------------------------------------------------------
CANARY = 0x7B7B                     # the 16-bit pattern around the caches


def carve(numel, dtype, pad=4096):
    """A cache buffer carved out of a larger device allocation with a canary pattern on both sides: (whole int16 view, the carved 1-D tensor)."""
    whole = torch.full((pad + numel + pad,), CANARY, dtype=torch.int16, device=DEV)
    return whole, whole[pad:pad + numel].view(dtype)


@pytest.mark.parametrize("n_new", [1, 3])
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_append_in_place_with_capacity_clamp(n_new, paged, dtype):
    gen = torch.Generator().manual_seed(70 + n_new)
    B, H, Hk, D, cap, page = 5, 8, 2, 64, 512, 128
    # room for all rows, the last row only just, one row too many, full, beyond the capacity (a bad length: nothing written, everything attended)
    lens = torch.tensor([100, cap - n_new, cap - 1, cap, cap + 7], dtype=torch.int32)
    q = randn(gen, B, n_new, H, D, dtype=dtype, std=1.0)
    kc, vc = randn(gen, B, cap, Hk, D, dtype=dtype), randn(gen, B, cap, Hk, D, dtype=dtype)
    kn, vn = randn(gen, B, n_new, Hk, D, dtype=dtype), randn(gen, B, n_new, Hk, D, dtype=dtype)
    bt = None
    if paged:
        kc, vc, bt = make_paged(gen, kc, vc, page)
    # the expected caches, on the CPU
    ke, ve = kc.clone(), vc.clone()
    for b in range(B):
        for t in range(n_new):
            pos = int(lens[b]) + t
            if pos >= cap:
                continue
            if paged:
                ke[int(bt[b, pos // page]), pos % page] = kn[b, t]
                ve[int(bt[b, pos // page]), pos % page] = vn[b, t]
            else:
                ke[b, pos] = kn[b, t]
                ve[b, pos] = vn[b, t]
    after = torch.clamp(lens + n_new, max=cap)
    scale = 1.0 / math.sqrt(D)
    ref = reference(q, ke, ve, after, bt, scale, True)
    k_whole, k_dev = carve(kc.numel(), dtype)
    v_whole, v_dev = carve(vc.numel(), dtype)
    k_dev, v_dev = k_dev.view(kc.shape), v_dev.view(vc.shape)
    k_dev.copy_(kc)
    v_dev.copy_(vc)
    lens_dev = lens.to(DEV)
    pad = (k_whole.numel() - kc.numel()) // 2
    for splits in (1, 2):
        k_dev.copy_(kc)
        v_dev.copy_(vc)
        out, lse = tfa.flash_attn_with_kvcache(q.to(DEV), k_dev, v_dev, kn.to(DEV), vn.to(DEV), cache_seqlens=lens_dev, block_table=None if bt is None else bt.to(DEV),
                                               causal=True, num_splits=splits, return_softmax_lse=True)
        torch.cuda.synchronize()
        assert torch.equal(lens_dev.cpu(), lens), "cache_seqlens was modified"
        for whole, dev, want, name in ((k_whole, k_dev, ke, "k"), (v_whole, v_dev, ve, "v")):
            assert torch.equal(dev.cpu().view(torch.int16), want.view(torch.int16)), f"{name}_cache differs from the expected cache (splits {splits})"
            w = whole.cpu()
            assert (w[:pad] == CANARY).all() and (w[pad + want.numel():] == CANARY).all(), f"a canary around {name}_cache was overwritten"
        assert_matches(out, lse, *ref, what=f"append n_new{n_new} paged={paged} {dtype} splits{splits}")


# ---- 8. no synchronisation: a captured decode step ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged", [False, True])
def test_captured_decode_step_replays_with_advanced_lengths(paged):
    gen = torch.Generator().manual_seed(8)
    dtype, B, H, Hk, D, cap = torch.bfloat16, 4, 8, 2, 128, 4096
    lens = torch.tensor([4000, 17, 2048, 0], dtype=torch.int32)
    kc, vc = randn(gen, B, cap, Hk, D, dtype=dtype), randn(gen, B, cap, Hk, D, dtype=dtype)
    bt = None
    if paged:
        kc, vc, bt = make_paged(gen, kc, vc, 256)
    steps = [(randn(gen, B, 1, H, D, dtype=dtype, std=1.0), randn(gen, B, 1, Hk, D, dtype=dtype), randn(gen, B, 1, Hk, D, dtype=dtype)) for _ in range(4)]
    k_dev, v_dev, lens_dev = kc.to(DEV), vc.to(DEV), lens.to(DEV)
    bt_dev = None if bt is None else bt.to(DEV)
    q_s, k_s, v_s = (t.to(DEV).clone() for t in steps[0])
    call = lambda: tfa.flash_attn_with_kvcache(q_s, k_dev, v_dev, k_s, v_s, cache_seqlens=lens_dev, block_table=bt_dev, causal=True, num_splits=0,
                                               return_softmax_lse=True)
    call()                                                                        # one warm-up call outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_s, lse_s = call()
    scale = 1.0 / math.sqrt(D)
    kc_cpu, vc_cpu, cur = kc.clone(), vc.clone(), lens.clone()
    for r in range(1, 4):
        qr, kr, vr = steps[r]
        q_s.copy_(qr.to(DEV))
        k_s.copy_(kr.to(DEV))
        v_s.copy_(vr.to(DEV))
        g.replay()
        torch.cuda.synchronize()
        for b in range(B):                                                        # the CPU mirror of the append
            pos = int(cur[b])
            if paged:
                kc_cpu[int(bt[b, pos // 256]), pos % 256] = kr[b, 0]
                vc_cpu[int(bt[b, pos // 256]), pos % 256] = vr[b, 0]
            else:
                kc_cpu[b, pos] = kr[b, 0]
                vc_cpu[b, pos] = vr[b, 0]
        ref = reference(qr, kc_cpu, vc_cpu, cur + 1, bt, scale, True)
        assert_matches(out_s, lse_s, *ref, what=f"replay {r} paged={paged}")
        lens_dev.add_(1)                                                          # the caller advances the lengths, in place on the device
        cur = cur + 1
    torch.cuda.synchronize()


# ---- 9. seeded random sweep ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(40))
def test_seeded_sweep(seed):
    gen = torch.Generator().manual_seed(9000 + seed)
    pick = lambda xs: xs[int(torch.randint(len(xs), (1,), generator=gen))]
    dtype = pick([torch.bfloat16, torch.float16])
    B = pick([1, 2, 3, 5])
    Hk = pick([1, 2, 4])
    H = Hk * pick([1, 2, 4, 8])
    D = pick([32, 40, 64, 72, 96, 104, 128])
    paged = pick([False, True])
    page = pick([64, 128, 192, 256])
    cap = page * pick([2, 3, 5]) if paged else pick([64, 100, 777, 1024, 1500])
    Nq = pick([1, 1, 1, 2, 5, 17, 130])
    causal = pick([False, True])
    splits = pick([0, 1, 2, 3, 8])
    lens = torch.randint(0, cap + 1, (B,), generator=gen).to(torch.int32)
    if seed % 5 == 0:
        lens[0] = cap
    if seed % 7 == 0:
        lens[-1] = 0
    q = randn(gen, B, Nq, H, D, dtype=dtype, std=1.0)
    kc, vc = randn(gen, B, cap, Hk, D, dtype=dtype), randn(gen, B, cap, Hk, D, dtype=dtype)
    for b in range(B):                                                            # large finite values behind every length
        kc[b, int(lens[b]):] = 30.0
        vc[b, int(lens[b]):] = -200.0
    scale = pick([1.0 / math.sqrt(D), 0.05])
    ref = reference(q, kc, vc, lens, None, scale, causal)
    bt = None
    if paged:
        kc, vc, bt = make_paged(gen, kc, vc, page)
    out, lse = run(q, kc, vc, lens, bt, causal=causal, splits=splits, scale=scale)
    assert_matches(out, lse, *ref, what=f"seed{seed} {dtype} B{B} H{H} Hk{Hk} D{D} paged={paged} page{page} cap{cap} Nq{Nq} causal={causal} splits{splits}")
