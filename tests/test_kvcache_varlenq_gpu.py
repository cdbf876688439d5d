"""GPU tests of ``flash_attn_with_kvcache(cu_seqlens_q=, max_seqlen_q=)`` (tfa_fwd_kvcache_varlen): packed ragged query rows over a K/V cache — the varlen-q form
of the KV-cache kernel, every sequence's first row and row count read and clamped on the device.  The bars are tests/test_kvcache_packgqa_gpu.py's (the same
kernel family: 16-bit out |d| <= 1e-2, LSE |d| <= 1e-4 * max(1, |ref|), +inf exactly on rows that see no key; q std 1.0, K/V std 0.5) against an fp64
per-sequence reference; wherever a row's arithmetic depends on its own sequence only — against the 4-D call — the requirement is bit identity, not a tolerance.
H8 Hk2 unless said otherwise.  Every case compares every element of every row that belongs to a sequence."""
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
H, HK = 8, 2
# the ragged batch of cases 2, 3 and 9: a sequence without rows, one without keys, len == nq (pure prefill), len < nq (rows that see nothing), 40 * 4 = 160 packed
# rows (two query blocks: the causal heavy / light pair), a length on a tile boundary
NQ = [1, 0, 7, 1, 40, 1, 5]
LENS = [300, 50, 7, 64, 129, 0, 3]
MAXQ = 40


def randn(gen, *shape, dtype, std=0.5):
    return (torch.randn(*shape, generator=gen, dtype=torch.float32) * std).to(dtype)


def cu_of(nq, start=0):
    c = [start]
    for n in nq:
        c.append(c[-1] + n)
    return torch.tensor(c, dtype=torch.int32)


def rows_of(cu, total_q, max_q):
    """(q0_b, nq_b) as every work item clamps them (include/tfa.h)."""
    res = []
    for b in range(len(cu) - 1):
        q0 = min(max(int(cu[b]), 0), total_q)
        res.append((q0, min(max(int(cu[b + 1]) - int(cu[b]), 0), min(max_q, total_q - q0))))
    return res


def gather_cache(cache, block_table, b, n):
    if block_table is None:
        return cache[b, :n]
    page = cache.shape[1]
    pages = [cache[int(block_table[b, i])] for i in range((n + page - 1) // page)]
    return torch.cat(pages, 0)[:n] if pages else cache[0, :0]


def reference(q, k_cache, v_cache, cu, lens, block_table, scale, causal, max_q, kd=None, vd=None):
    """fp64 attention of every sequence's rows over its own (decoded, descaled) keys: out (total_q, H, D), lse (H, total_q), owned (total_q,) — the rows that belong
    to a sequence; rows that see no key: out = 0, lse = +inf."""
    q, k_cache, v_cache = q.double().cpu(), k_cache.cpu().double(), v_cache.cpu().double()
    bt = None if block_table is None else block_table.cpu()
    total_q, Hq, D = q.shape
    Hk = k_cache.shape[2]
    G = Hq // Hk
    cap = k_cache.shape[1] * (bt.shape[1] if bt is not None else 1)
    B = len(cu) - 1
    kd = torch.ones(B, Hk, dtype=torch.float64) if kd is None else kd.double().cpu()
    vd = torch.ones(B, Hk, dtype=torch.float64) if vd is None else vd.double().cpu()
    out = torch.zeros(total_q, Hq, D, dtype=torch.float64)
    lse = torch.full((Hq, total_q), math.inf, dtype=torch.float64)
    owned = torch.zeros(total_q, dtype=torch.bool)
    for b, (q0, nq) in enumerate(rows_of(cu, total_q, max_q)):
        owned[q0:q0 + nq] = True
        n = min(max(int(lens[b]), 0), cap)
        if n == 0 or nq == 0:
            continue
        k = (gather_cache(k_cache, bt, b, n) * kd[b].view(1, Hk, 1)).repeat_interleave(G, dim=1)
        v = (gather_cache(v_cache, bt, b, n) * vd[b].view(1, Hk, 1)).repeat_interleave(G, dim=1)
        s = torch.einsum("qhd,khd->hqk", q[q0:q0 + nq], k) * scale
        if causal:
            i = torch.arange(nq).view(nq, 1)
            j = torch.arange(n).view(1, n)
            s = s.masked_fill(j > i + (n - nq), -math.inf)
        l = torch.logsumexp(s, dim=-1)
        seen = torch.isfinite(l)
        p = torch.exp(s - torch.where(seen, l, torch.zeros_like(l)).unsqueeze(-1))
        p = torch.where(seen.unsqueeze(-1), p, torch.zeros_like(p))
        out[q0:q0 + nq] = torch.einsum("hqk,khd->qhd", p, v)
        lse[:, q0:q0 + nq] = torch.where(seen, l, torch.full_like(l, math.inf))
    return out, lse, owned


def assert_matches(out, lse, ref, what=""):
    ref_out, ref_lse, owned = ref
    out, lse = out.double().cpu()[owned], lse.double().cpu()[:, owned]
    ref_out, ref_lse = ref_out[owned], ref_lse[:, owned]
    assert out.shape == ref_out.shape and lse.shape == ref_lse.shape
    assert not torch.isnan(out).any(), f"{what}: NaN in out"
    assert not torch.isnan(lse).any(), f"{what}: NaN in lse"
    err = (out - ref_out).abs().max().item() if out.numel() else 0.0
    inf_ref = torch.isinf(ref_lse)
    assert torch.equal(torch.isinf(lse) & (lse > 0), inf_ref), f"{what}: lse = +inf on other rows than the reference"
    fin = ~inf_ref
    rel = ((lse[fin] - ref_lse[fin]).abs() / ref_lse[fin].abs().clamp(min=1.0)).max().item() if fin.any() else 0.0
    print(f"{what}: max|d out| = {err:.3e} (bar {OUT_BAR}), max LSE err = {rel:.3e} (bar {LSE_BAR}), empty rows = {int(inf_ref.sum())}")
    assert err <= OUT_BAR, f"{what}: max|d out| = {err}"
    assert rel <= LSE_BAR, f"{what}: LSE error {rel}"
    if inf_ref.any():
        assert (out.transpose(0, 1)[inf_ref] == 0).all(), f"{what}: out != 0 on rows that see no key"


def make_paged(gen, kc, vc, page, spare=3, fill=None):
    """tests/test_kvcache_packgqa_gpu.py's: a contiguous (B, cap, Hk, D) cache scattered into pages through a seeded shuffled block table; spare pages hold garbage."""
    B, cap, Hk, D = kc.shape
    mb = cap // page
    nb = B * mb + spare
    perm = torch.randperm(nb, generator=gen)[: B * mb].view(B, mb)
    if kc.dtype == E4M3:
        kp = torch.full((nb, page, Hk, D), 0x7F, dtype=torch.uint8).view(E4M3)
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


def run(q, kc, vc, cu, lens, max_q, bt=None, causal=False, splits=1, scale=None, pack=None, kd=None, vd=None):
    d = lambda t: None if t is None else t.to(DEV)
    out, lse = tfa.flash_attn_with_kvcache(d(q), d(kc), d(vc), cache_seqlens=d(lens), block_table=d(bt), softmax_scale=scale, causal=causal, num_splits=splits,
                                           return_softmax_lse=True, pack_gqa=pack, k_descale=d(kd), v_descale=d(vd), cu_seqlens_q=d(cu), max_seqlen_q=max_q)
    torch.cuda.synchronize()
    assert tuple(out.shape) == tuple(q.shape) and tuple(lse.shape) == (q.shape[1], q.shape[0])
    return out, lse


def run4d(q4, kc, vc, lens, bt=None, causal=False, splits=1, scale=None, pack=True, kd=None, vd=None):
    d = lambda t: None if t is None else t.to(DEV)
    out, lse = tfa.flash_attn_with_kvcache(d(q4), d(kc), d(vc), cache_seqlens=d(lens), block_table=d(bt), softmax_scale=scale, causal=causal, num_splits=splits,
                                           return_softmax_lse=True, pack_gqa=pack, k_descale=d(kd), v_descale=d(vd))
    torch.cuda.synchronize()
    return out, lse


def ragged(gen, dtype, D, cap=512, heads=(H, HK)):
    hq, hk = heads
    cu, lens = cu_of(NQ), torch.tensor(LENS, dtype=torch.int32)
    q = randn(gen, int(cu[-1]), hq, D, dtype=dtype, std=1.0)
    kc, vc = randn(gen, len(NQ), cap, hk, D, dtype=dtype), randn(gen, len(NQ), cap, hk, D, dtype=dtype)
    return q, kc, vc, cu, lens


# ---- 1. equal lengths give the 4-D call's bits ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [64, 128])
def test_equal_lengths_give_the_same_bits(dtype, D):
    gen = torch.Generator().manual_seed(100 + D)
    B, cap = 3, 1024
    lens = torch.tensor([200, 64, 777], dtype=torch.int32)
    kc, vc = randn(gen, B, cap, HK, D, dtype=dtype), randn(gen, B, cap, HK, D, dtype=dtype)
    for Nq in (1, 3):
        q4 = randn(gen, B, Nq, H, D, dtype=dtype, std=1.0)
        q = q4.reshape(B * Nq, H, D)
        cu = cu_of([Nq] * B)
        for causal in (True, False):
            for splits in (1, 3):
                for pack in (True, False):
                    out, lse = run(q, kc, vc, cu, lens, Nq, causal=causal, splits=splits, pack=pack)
                    o4, l4 = run4d(q4, kc, vc, lens, causal=causal, splits=splits, pack=pack)
                    what = f"{dtype} D{D} Nq{Nq} causal={causal} splits{splits} pack={pack}"
                    assert torch.equal(out.reshape(B, Nq, H, D), o4), f"{what}: out differs from the 4-D call in bits"
                    assert torch.equal(lse.view(H, B, Nq).transpose(0, 1), l4), f"{what}: lse differs from the 4-D call in bits"


# ---- 2. ragged, against fp64 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page", [0, 64, 128])
@pytest.mark.parametrize("causal", [True, False])
def test_ragged_against_fp64(page, causal):
    gen = torch.Generator().manual_seed(200 + page)
    dtype, D = torch.bfloat16, 64
    q, kc, vc, cu, lens = ragged(gen, dtype, D)
    bt = None
    if page:
        kc, vc, bt = make_paged(gen, kc, vc, page)
    scale = 1.0 / math.sqrt(D)
    ref = reference(q, kc, vc, cu, lens, bt, scale, causal, MAXQ)
    assert ref[2].all()
    if causal:                                          # len 3 < nq 5: the first two rows see nothing; len 0: none does
        assert torch.isinf(ref[1][:, 50:52]).all() and torch.isfinite(ref[1][:, 52:55]).all() and torch.isinf(ref[1][:, 49]).all()
    for splits in (1, 3):
        out, lse = run(q, kc, vc, cu, lens, MAXQ, bt, causal=causal, splits=splits, scale=scale)
        assert_matches(out, lse, ref, what=f"ragged page{page} causal={causal} splits{splits}")


# ---- 3. ragged: every sequence has the bits of the 4-D call on that sequence alone --------------------------------------------------------------------
@pytest.mark.parametrize("pack", [True, False])
@pytest.mark.parametrize("causal", [True, False])
def test_ragged_per_sequence_bits(pack, causal):
    gen = torch.Generator().manual_seed(300)
    dtype, D = torch.float16, 128
    q, kc, vc, cu, lens = ragged(gen, dtype, D)
    for splits in (1, 3):
        out, lse = run(q, kc, vc, cu, lens, MAXQ, causal=causal, splits=splits, pack=pack)
        for b, (q0, nq) in enumerate(rows_of(cu, q.shape[0], MAXQ)):
            if nq == 0:
                continue
            o1, l1 = run4d(q[q0:q0 + nq].unsqueeze(0), kc[b:b + 1], vc[b:b + 1], lens[b:b + 1], causal=causal, splits=splits, pack=pack)
            what = f"sequence {b} (nq {nq}, len {int(lens[b])}) causal={causal} splits{splits} pack={pack}"
            assert torch.equal(out[q0:q0 + nq], o1[0]), f"{what}: out differs in bits"
            assert torch.equal(lse[:, q0:q0 + nq], l1[0]), f"{what}: lse differs in bits"


# ---- 4. group sizes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [(8, 8), (8, 1), (6, 2)])
def test_group_sizes(heads):
    """H == Hk (MHA: the unpacked instantiations), MQA, and G = 3; pack_gqa False against True."""
    gen = torch.Generator().manual_seed(400 + heads[0] * 10 + heads[1])
    dtype, D = torch.bfloat16, 64
    q, kc, vc, cu, lens = ragged(gen, dtype, D, heads=heads)
    scale = 1.0 / math.sqrt(D)
    ref = reference(q, kc, vc, cu, lens, None, scale, True, MAXQ)
    for splits in (1, 2):
        on, lse_on = run(q, kc, vc, cu, lens, MAXQ, causal=True, splits=splits, scale=scale, pack=True)
        assert_matches(on, lse_on, ref, what=f"H{heads[0]} Hk{heads[1]} pack=True splits{splits}")
        off, lse_off = run(q, kc, vc, cu, lens, MAXQ, causal=True, splits=splits, scale=scale, pack=False)
        assert_matches(off, lse_off, ref, what=f"H{heads[0]} Hk{heads[1]} pack=False splits{splits}")
        d = (on.float() - off.float()).abs().max().item()
        fin = torch.isfinite(lse_on)
        assert torch.equal(fin, torch.isfinite(lse_off))
        dl = ((lse_on[fin] - lse_off[fin]).abs() / lse_on[fin].abs().clamp(min=1.0)).max().item()
        print(f"H{heads[0]} Hk{heads[1]} splits{splits}: max|True - False| = {d:.3e}, LSE {dl:.3e}")
        assert d <= OUT_BAR and dl <= LSE_BAR
        if heads[0] == heads[1]:
            assert torch.equal(on, off) and torch.equal(lse_on, lse_off), "H == Hk: True and False are one launch"


# ---- 5. fp8 cache -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged", [False, True])
def test_fp8_cache(paged):
    gen = torch.Generator().manual_seed(500)
    dtype, D, cap, B = torch.bfloat16, 128, 512, len(NQ)
    cu, lens = cu_of(NQ), torch.tensor(LENS, dtype=torch.int32)
    q = randn(gen, int(cu[-1]), H, D, dtype=dtype, std=1.0)
    kd = 0.002 + 0.018 * torch.rand(B, HK, generator=gen, dtype=torch.float32)
    vd = 0.002 + 0.018 * torch.rand(B, HK, generator=gen, dtype=torch.float32)
    quant = lambda x, d: (x.float() / d.view(B, 1, HK, 1)).clamp(-448.0, 448.0).to(E4M3)
    k8 = quant(randn(gen, B, cap, HK, D, dtype=torch.float32), kd)
    v8 = quant(randn(gen, B, cap, HK, D, dtype=torch.float32), vd)
    for b in range(B):                                                            # the NaN code behind every length
        k8.view(torch.uint8)[b, int(lens[b]):] = 0x7F
        v8.view(torch.uint8)[b, int(lens[b]):] = 0x7F
    scale = 1.0 / math.sqrt(D)
    ref = reference(q, k8, v8, cu, lens, None, scale, True, MAXQ, kd, vd)
    k16, v16 = k8.to(dtype), v8.to(dtype)                                         # exact: every finite e4m3 value is a bf16
    bt, kk, vv = None, k8, v8
    if paged:
        state = gen.get_state()
        kk, vv, bt = make_paged(gen, k8, v8, 128)
        gen.set_state(state)
        k16, v16, bt16 = make_paged(gen, k16, v16, 128, fill=float("nan"))
        assert torch.equal(bt, bt16)
    for splits in (1, 3):
        out, lse = run(q, kk, vv, cu, lens, MAXQ, bt, causal=True, splits=splits, scale=scale, kd=kd, vd=vd)
        assert_matches(out, lse, ref, what=f"fp8 paged={paged} splits{splits}")
        one, lse_one = run(q, kk, vv, cu, lens, MAXQ, bt, causal=True, splits=splits, scale=scale)
        out16, lse16 = run(q, k16, v16, cu, lens, MAXQ, bt, causal=True, splits=splits, scale=scale)
        assert torch.equal(one, out16) and torch.equal(lse_one, lse16), "fp8 at descale 1.0 and the 16-bit call over the converted caches differ in bits"


# ---- 6 / 7. the C ABI over tensors carved out of larger allocations -------------------------------------------------------------------------------------
CANARY = 0x7B7B
LSE_CANARY = -7.0


class Carved:
    """q, out (laid out like q, or dense (H, total_q, D)), lse and optionally a workspace, each inside a larger allocation: NaN around q, canaries around and IN
    out / lse / the workspace."""

    def __init__(self, q, dense_out, ws_floats=0):
        self.total_q, self.Hq, self.D = q.shape
        n = q.numel()
        self.pad = pad = 64 * self.Hq * self.D
        self.q_whole = torch.full((pad + n + pad,), float("nan"), dtype=q.dtype, device=DEV)
        self.q = self.q_whole[pad:pad + n].view(q.shape)
        self.q.copy_(q)
        self.q_cpu = q
        self.o_whole = torch.full((pad + n + pad,), CANARY, dtype=torch.int16, device=DEV)
        flat = self.o_whole[pad:pad + n].view(q.dtype)
        self.out = flat.view(self.Hq, self.total_q, self.D).transpose(0, 1) if dense_out else flat.view(q.shape)      # (total_q, H, D) either way
        self.nl = self.Hq * self.total_q
        self.lse_whole = torch.full((64 + self.nl + 64,), LSE_CANARY, dtype=torch.float32, device=DEV)
        self.lse = self.lse_whole[64:64 + self.nl].view(self.Hq, self.total_q)
        self.ws_floats = ws_floats
        self.ws_whole = torch.full((64 + ws_floats + 64,), LSE_CANARY, dtype=torch.float32, device=DEV) if ws_floats else None

    def call(self, kc, vc, cu, lens, max_q, bt, causal, splits, scale, pack=_lib.TFA_PACK_GQA_AUTO):
        p = _lib.TfaKvcacheParams()
        p.q, p.out, p.lse = self.q.data_ptr(), self.out.data_ptr(), self.lse.data_ptr()
        p.k_cache, p.v_cache, p.cache_seqlens = kc.data_ptr(), vc.data_ptr(), lens.data_ptr()
        p.B, p.H, p.Hk, p.Nq, p.D = cu.numel() - 1, self.Hq, kc.shape[2], 0, self.D
        if bt is not None:
            p.block_table, p.block_table_stride = bt.data_ptr(), bt.stride(0)
            p.page_size, p.num_pages, p.capacity = kc.shape[1], kc.shape[0], bt.shape[1] * kc.shape[1]
        else:
            p.capacity = kc.shape[1]
        p.q_stride[0], p.q_stride[1], p.q_stride[2] = 0, self.q.stride(1), self.q.stride(0)
        p.o_stride[0], p.o_stride[1], p.o_stride[2] = 0, self.out.stride(1), self.out.stride(0)
        for name, t in (("k_stride", kc), ("v_stride", vc)):
            arr = getattr(p, name)
            arr[0], arr[1], arr[2] = t.stride(0), t.stride(2), t.stride(1)
        p.softmax_scale, p.is_causal, p.dtype = float(scale), 1 if causal else 0, ops._DT[self.q.dtype]
        vq = _lib.TfaKvcacheVarlenQ()
        vq.cu_seqlens_q, vq.max_seqlen_q, vq.total_q = cu.data_ptr(), max_q, self.total_q
        L = _lib.lib()
        need = L.tfa_fwd_kvcache_varlen_workspace(C.byref(p), C.byref(vq), None, pack, splits)
        assert need == self.ws_floats, (need, self.ws_floats)
        ws = self.ws_whole[64:].data_ptr() if self.ws_whole is not None else None
        with torch.cuda.device(self.q.device):
            _lib.check(L.tfa_fwd_kvcache_varlen(C.byref(p), C.byref(vq), None, pack, splits, ws, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()

    def check_untouched(self, owned):
        pad, n = self.pad, self.q_cpu.numel()
        w = self.o_whole.cpu()
        assert (w[:pad] == CANARY).all() and (w[pad + n:] == CANARY).all(), "a guard band around out was overwritten"
        lw = self.lse_whole.cpu()
        assert (lw[:64] == LSE_CANARY).all() and (lw[64 + self.nl:] == LSE_CANARY).all(), "a guard band around lse was overwritten"
        qw = self.q_whole.cpu()
        assert torch.isnan(qw[:pad]).all() and torch.isnan(qw[pad + n:]).all(), "the surroundings of q were written"
        assert torch.equal(self.q.cpu().view(torch.int16), self.q_cpu.view(torch.int16)), "q was written"
        if self.ws_whole is not None:
            ww = self.ws_whole.cpu()
            assert (ww[:64] == LSE_CANARY).all() and (ww[64 + self.ws_floats:] == LSE_CANARY).all(), "a guard band around the workspace was overwritten"
        free = ~owned
        if free.any():                                 # rows outside every sequence keep the canary
            assert (self.out.cpu().view(torch.int16)[free] == CANARY).all(), "a row of out outside every sequence was written"
            assert (self.lse.cpu()[:, free] == LSE_CANARY).all(), "a row of lse outside every sequence was written"


@pytest.mark.parametrize("paged", [False, True])
def test_nothing_leaks_in_or_out(paged):
    """NaN behind every length, in unreferenced pages and in the q rows outside every sequence (two in front of cu[0], three behind cu[B])."""
    gen = torch.Generator().manual_seed(600)
    dtype, D, cap, B = torch.bfloat16, 64, 512, len(NQ)
    cu, lens = cu_of(NQ, start=2), torch.tensor(LENS, dtype=torch.int32)
    total_q = int(cu[-1]) + 3
    q = randn(gen, total_q, H, D, dtype=dtype, std=1.0)
    kc, vc = randn(gen, B, cap, HK, D, dtype=dtype), randn(gen, B, cap, HK, D, dtype=dtype)
    scale = 1.0 / math.sqrt(D)
    ref = reference(q, kc, vc, cu, lens, None, scale, True, MAXQ)
    assert int((~ref[2]).sum()) == 5
    q[~ref[2]] = float("nan")
    for b in range(B):
        kc[b, int(lens[b]):] = float("nan")
        vc[b, int(lens[b]):] = float("nan")
    bt = None
    if paged:
        kc, vc, bt = make_paged(gen, kc, vc, 128, fill=float("nan"))
    for splits in (1, 3):                               # the Python call: fresh out / lse
        out, lse = run(q, kc, vc, cu, lens, MAXQ, bt, causal=True, splits=splits, scale=scale)
        assert_matches(out, lse, ref, what=f"NaN around, paged={paged} splits{splits}")
    kc_d, vc_d, cu_d, lens_d = kc.to(DEV), vc.to(DEV), cu.to(DEV), lens.to(DEV)
    bt_d = None if bt is None else bt.to(DEV)
    c = Carved(q, dense_out=False)                      # one chunk: out laid out like q
    c.call(kc_d, vc_d, cu_d, lens_d, MAXQ, bt_d, True, 1, scale)
    assert_matches(c.out, c.lse, ref, what=f"C ABI splits1 paged={paged}")
    c.check_untouched(ref[2])
    c = Carved(q, dense_out=True, ws_floats=3 * H * total_q * (D + 1))
    c.call(kc_d, vc_d, cu_d, lens_d, MAXQ, bt_d, True, 3, scale)
    assert_matches(c.out, c.lse, ref, what=f"C ABI splits3 paged={paged}")
    c.check_untouched(torch.ones(total_q, dtype=torch.bool))      # (the merge writes every row of the dense out: the bands only)


@pytest.mark.parametrize("pack", [_lib.TFA_PACK_GQA_ON, _lib.TFA_PACK_GQA_OFF])
@pytest.mark.parametrize("causal", [True, False])
def test_clamping(pack, causal):
    """A cu_seqlens_q whose last entry exceeds total_q and an nq_b above max_seqlen_q: only the clamped rows are computed — 12 rows asked with max_seqlen_q = 8 are
    rows 5..12 (8 rows, the causal shift len - 8), 13 rows asked at row 17 of 20 are 3 — and they match the reference of the clamped problem; rows 13..16 belong
    to no sequence and keep the canary."""
    gen = torch.Generator().manual_seed(700)
    dtype, D, cap, total_q, max_q = torch.float16, 64, 256, 20, 8
    cu = torch.tensor([0, 5, 17, 30], dtype=torch.int32)
    lens = torch.tensor([100, 200, 64], dtype=torch.int32)
    assert rows_of(cu, total_q, max_q) == [(0, 5), (5, 8), (17, 3)]
    q = randn(gen, total_q, H, D, dtype=dtype, std=1.0)
    kc, vc = randn(gen, 3, cap, HK, D, dtype=dtype), randn(gen, 3, cap, HK, D, dtype=dtype)
    scale = 1.0 / math.sqrt(D)
    ref = reference(q, kc, vc, cu, lens, None, scale, causal, max_q)
    assert ref[2].tolist() == [True] * 13 + [False] * 4 + [True] * 3
    c = Carved(q, dense_out=False)
    c.call(kc.to(DEV), vc.to(DEV), cu.to(DEV), lens.to(DEV), max_q, None, causal, 1, scale, pack)
    assert_matches(c.out, c.lse, ref, what=f"clamped pack={pack} causal={causal}")
    c.check_untouched(ref[2])


# ---- 8. a captured step: packed append + rotary + this call ----------------------------------------------------------------------------------------------
def test_captured_step_follows_in_place_updates():
    gen = torch.Generator().manual_seed(800)
    dtype, D, cap, page, B, total_q, max_q = torch.bfloat16, 64, 512, 128, 4, 24, 16
    kc, vc = randn(gen, B, cap, HK, D, dtype=dtype), randn(gen, B, cap, HK, D, dtype=dtype)
    kc, vc, bt = make_paged(gen, kc, vc, page)
    pos = torch.arange(cap, dtype=torch.float32).view(cap, 1) * (10000.0 ** (-torch.arange(0, D // 2, dtype=torch.float32) / (D // 2))).view(1, D // 2)
    cos, sin = pos.cos().to(DEV), pos.sin().to(DEV)
    steps = [([1, 16, 1, 6], [100, 0, 300, 64]), ([8, 1, 15, 0], [17, 129, 200, 5]), ([6, 6, 6, 6], [0, 63, 250, 496])]
    k_dev, v_dev = kc.to(DEV), vc.to(DEV)
    cu_dev, before_dev, bt_dev = cu_of(steps[0][0]).to(DEV), torch.tensor(steps[0][1], dtype=torch.int32, device=DEV), bt.to(DEV)
    after_dev = torch.zeros(B, dtype=torch.int32, device=DEV)
    q_s = randn(gen, total_q, H, D, dtype=dtype, std=1.0).to(DEV)
    k_s, v_s = randn(gen, total_q, HK, D, dtype=dtype).to(DEV), randn(gen, total_q, HK, D, dtype=dtype).to(DEV)

    def step(kcache, vcache):
        qr = ops.apply_rotary_emb(q_s, cos, sin, cu_seqlens=cu_dev, seqlen_offsets=before_dev)
        ops.kvcache_append_varlen(k_s, v_s, kcache, vcache, cu_dev, before_dev, bt_dev, rotary_cos=cos, rotary_sin=sin)
        after_dev.copy_(before_dev + (cu_dev[1:] - cu_dev[:-1]))
        return tfa.flash_attn_with_kvcache(qr, kcache, vcache, cache_seqlens=after_dev, block_table=bt_dev, causal=True, num_splits=2, return_softmax_lse=True,
                                           cu_seqlens_q=cu_dev, max_seqlen_q=max_q)

    with torch.no_grad():
        step(k_dev.clone(), v_dev.clone())              # warm-up outside the capture, on copies
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out_s, lse_s = step(k_dev, v_dev)
        for r, (nq, lens) in enumerate(steps):
            assert sum(nq) == total_q and max(nq) <= max_q
            cu_dev.copy_(cu_of(nq).to(DEV))
            before_dev.copy_(torch.tensor(lens, dtype=torch.int32, device=DEV))
            bt_dev.copy_(bt_dev.flip(0) if r == 1 else bt_dev)      # the table, overwritten in place
            q_s.copy_(randn(gen, total_q, H, D, dtype=dtype, std=1.0).to(DEV))
            k_s.copy_(randn(gen, total_q, HK, D, dtype=dtype).to(DEV))
            v_s.copy_(randn(gen, total_q, HK, D, dtype=dtype).to(DEV))
            k_e, v_e = k_dev.clone(), v_dev.clone()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            out_r, lse_r = out_s.clone(), lse_s.clone()
            out_e, lse_e = step(k_e, v_e)               # the eager call on the new values
            torch.cuda.synchronize()
            assert torch.equal(out_r, out_e) and torch.equal(lse_r, lse_e), f"replay {r} differs from the eager step in bits"
            assert torch.equal(k_dev.view(torch.int16), k_e.view(torch.int16)) and torch.equal(v_dev.view(torch.int16), v_e.view(torch.int16))
            assert torch.isfinite(lse_r).any() and not torch.isnan(out_r).any()


# ---- 9. the unified step agrees with the paged varlen route ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False])
def test_agrees_with_flash_attn_varlen_func_over_the_same_pages(causal):
    """Different kernels and rounding rules: the bars, not the bits."""
    gen = torch.Generator().manual_seed(900)
    dtype, D = torch.bfloat16, 64
    q, kc, vc, cu, lens = ragged(gen, dtype, D)
    kp, vp, bt = make_paged(gen, kc, vc, 128)
    scale = 1.0 / math.sqrt(D)
    out, lse = run(q, kp, vp, cu, lens, MAXQ, bt, causal=causal, splits=1, scale=scale)
    ref = reference(q, kp, vp, cu, lens, bt, scale, causal, MAXQ)
    assert_matches(out, lse, ref, what=f"this call, causal={causal}")
    cu_k = cu_of(LENS)
    with torch.no_grad():
        o2, l2 = ops.flash_attn_varlen_fwd(q.to(DEV), kp.to(DEV), vp.to(DEV), cu.to(DEV), cu_k.to(DEV), MAXQ, max(LENS), causal, scale, block_table=bt.to(DEV))
    torch.cuda.synchronize()
    assert_matches(o2, l2, ref, what=f"the paged varlen route, causal={causal}")
    d = (out.float() - o2.float()).abs().max().item()
    fin = torch.isfinite(lse)
    assert torch.equal(fin, torch.isfinite(l2)), "+inf on different rows"
    dl = ((lse[fin] - l2[fin]).abs() / lse[fin].abs().clamp(min=1.0)).max().item()
    print(f"causal={causal}: max|kvcache varlen-q - paged varlen| = {d:.3e} (bar {OUT_BAR}), LSE {dl:.3e} (bar {LSE_BAR})")
    assert d <= OUT_BAR and dl <= LSE_BAR
