"""GPU tests of the scheduled packed-q K/V-cache call: ``get_scheduler_metadata`` (tfa_kvcache_varlen_schedule — the work list built on the device) and
``flash_attn_with_kvcache(cu_seqlens_q=, max_seqlen_q=, scheduler_metadata=)`` (tfa_fwd_kvcache_varlen_sched — the scheduled form of the KV-cache kernel).  The list
is compared with its host restatement word for word; the attention call with the unscheduled call bit for bit (a block's arithmetic does not depend on the work
item that runs it) and with the fp64 reference at tests/test_kvcache_varlenq_gpu.py's bars (16-bit out |d| <= 1e-2, LSE |d| <= 1e-4 * max(1, |ref|), +inf exactly on
rows that see no key); lists that do not belong to the batch must leave everything outside the owned rows untouched.  Helpers and the ragged batch are that
file's.  H8 Hk2 unless said otherwise."""
import ctypes as C
import math

import pytest
import torch

import kvcache_sched_ref as R
import test_kvcache_varlenq_gpu as V
import tiny_flash_attention_amd as tfa
from tiny_flash_attention_amd import _lib

pytestmark = pytest.mark.gpu

DEV, H, HK, E4M3 = V.DEV, V.H, V.HK, V.E4M3
NQ, LENS, MAXQ = V.NQ, V.LENS, V.MAXQ
# a batch whose only multi-block sequence has an odd block count: 70 * 4 = 280 packed rows are three blocks — under causal the pair (2, 0) and block 1 alone
ODD_NQ, ODD_LENS, ODD_MAXQ = [2, 70, 0, 3], [130, 200, 64, 3], 70
randn, cu_of, reference, assert_matches, make_paged = V.randn, V.cu_of, V.reference, V.assert_matches, V.make_paged


def metadata(cu, max_q, total_q, heads=(H, HK), causal=False, pack=None, out=None):
    md = tfa.get_scheduler_metadata(cu.to(DEV), max_q, total_q, heads[0], heads[1], causal=causal, pack_gqa=pack, out=out)
    torch.cuda.synchronize()
    return md


def run_sched(q, kc, vc, cu, lens, max_q, bt=None, causal=False, splits=1, scale=None, pack=None, kd=None, vd=None, md=None):
    d = lambda t: None if t is None else t.to(DEV)
    if md is None:
        md = metadata(cu, max_q, q.shape[0], (q.shape[1], kc.shape[2]), causal, pack)
    out, lse = tfa.flash_attn_with_kvcache(d(q), d(kc), d(vc), cache_seqlens=d(lens), block_table=d(bt), softmax_scale=scale, causal=causal, num_splits=splits,
                                           return_softmax_lse=True, pack_gqa=pack, k_descale=d(kd), v_descale=d(vd), cu_seqlens_q=d(cu), max_seqlen_q=max_q,
                                           scheduler_metadata=md)
    torch.cuda.synchronize()
    assert tuple(out.shape) == tuple(q.shape) and tuple(lse.shape) == (q.shape[1], q.shape[0])
    return out, lse


def batch(gen, dtype, D, nq, lens, cap=512, heads=(H, HK)):
    cu = cu_of(nq)
    q = randn(gen, int(cu[-1]), heads[0], D, dtype=dtype, std=1.0)
    kc, vc = randn(gen, len(nq), cap, heads[1], D, dtype=dtype), randn(gen, len(nq), cap, heads[1], D, dtype=dtype)
    return q, kc, vc, cu, torch.tensor(lens, dtype=torch.int32)


def assert_same_bits(got, want, owned, what):
    assert torch.equal(got[0][owned], want[0][owned]), f"{what}: out differs from the unscheduled call in bits"
    assert torch.equal(got[1][:, owned], want[1][:, owned]), f"{what}: lse differs from the unscheduled call in bits"


# ---- 1. the list ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pack", [None, False])
@pytest.mark.parametrize("causal", [True, False])
def test_schedule_contents(pack, causal):
    """Header and rows, word for word, in the fixed order: the ragged batch, the odd batch, a cu_seqlens_q with out-of-range entries (clamped as the attention
    kernel clamps), one that starts behind row 0, and 600 sequences (the scan's carry across its 256-sequence strides)."""
    gp = 1 if pack is False else H // HK
    many = [(i * 7) % 5 if i % 3 else (130 if i % 30 == 0 else 0) for i in range(600)]
    cases = [(cu_of(NQ), MAXQ, sum(NQ)), (cu_of(ODD_NQ), ODD_MAXQ, sum(ODD_NQ)), (torch.tensor([0, 5, 17, 30], dtype=torch.int32), 8, 20),
             (torch.tensor([-4, 3, 3, 90, 95], dtype=torch.int32), 33, 91), (cu_of(NQ, start=2), MAXQ, sum(NQ) + 5), (cu_of(many), 130, sum(many))]
    for cu, max_q, total_q in cases:
        want = R.schedule(cu.tolist(), max_q, total_q, gp, causal)
        md = metadata(cu, max_q, total_q, causal=causal, pack=pack).cpu()
        what = f"B{cu.numel() - 1} max_q{max_q} total_q{total_q} causal={causal} pack={pack}"
        assert md.dtype == torch.int32 and md.numel() == R.HDR + 2 * want[6], what
        assert md[:len(want)].tolist() == want, what
    # out= reuses a buffer: the same words over whatever it held
    cu = cu_of(NQ)
    buf = torch.full((R.HDR + 2 * R.bound_of(len(NQ), MAXQ, sum(NQ), gp, causal),), -77, dtype=torch.int32, device=DEV)
    md = metadata(cu, MAXQ, sum(NQ), causal=causal, pack=pack, out=buf)
    want = R.schedule(cu.tolist(), MAXQ, sum(NQ), gp, causal)
    assert md is buf and md[:len(want)].tolist() == want and (md[len(want):] == -77).all()      # rows behind n_items are not written
    # a cu_seqlens_q that is not monotonic describes more items than the bound (three sequences claim nearly all 300 rows each): the list ends at the bound,
    # n_items says so, and nothing is written behind the buffer
    cu, max_q, total_q = torch.tensor([0, 300, 1, 300, 2, 300], dtype=torch.int32), 300, 300
    want = R.schedule(cu.tolist(), max_q, total_q, gp, causal)
    described = sum(R.items_of(R.blocks_of(n, gp), causal) for _, n in R.rows_of(cu.tolist(), total_q, max_q))
    assert want[0] == min(described, want[6]) and (gp == 1 or described > want[6])
    size = R.HDR + 2 * want[6]
    whole = torch.full((16 + size + 16,), -77, dtype=torch.int32, device=DEV)
    md = metadata(cu, max_q, total_q, causal=causal, pack=pack, out=whole[16:16 + size])
    assert md[:len(want)].tolist() == want and (md[len(want):] == -77).all()
    assert (whole[:16] == -77).all() and (whole[16 + size:] == -77).all(), "a guard band around the metadata was overwritten"


# ---- 2. the unscheduled call's bits -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [64, 128])
def test_same_bits_as_the_unscheduled_call(dtype, D):
    gen = torch.Generator().manual_seed(1100 + D)
    q, kc, vc, cu, lens = batch(gen, dtype, D, NQ, LENS)
    owned = torch.ones(q.shape[0], dtype=torch.bool)
    for page in (0, 64, 128):
        kk, vv, bt = (kc, vc, None) if not page else make_paged(gen, kc, vc, page)
        for causal in (True, False):
            for pack in (True, False):
                md = metadata(cu, MAXQ, q.shape[0], causal=causal, pack=pack)                 # one list, every split count (as every layer of a step)
                for splits in (1, 3):
                    got = run_sched(q, kk, vv, cu, lens, MAXQ, bt, causal=causal, splits=splits, pack=pack, md=md)
                    want = V.run(q, kk, vv, cu, lens, MAXQ, bt, causal=causal, splits=splits, pack=pack)
                    assert_same_bits(got, want, owned, f"{dtype} D{D} page{page} causal={causal} pack={pack} splits{splits}")
    q, kc, vc, cu, lens = batch(gen, dtype, D, ODD_NQ, ODD_LENS)                               # three blocks: the middle one alone
    owned = torch.ones(q.shape[0], dtype=torch.bool)
    for causal in (True, False):
        for pack in (True, False):
            for splits in (1, 3):
                got = run_sched(q, kc, vc, cu, lens, ODD_MAXQ, causal=causal, splits=splits, pack=pack)
                want = V.run(q, kc, vc, cu, lens, ODD_MAXQ, causal=causal, splits=splits, pack=pack)
                assert_same_bits(got, want, owned, f"odd batch {dtype} D{D} causal={causal} pack={pack} splits{splits}")


@pytest.mark.parametrize("paged", [False, True])
def test_fp8_cache(paged):
    gen = torch.Generator().manual_seed(1200)
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
    bt = None
    if paged:
        k8, v8, bt = make_paged(gen, k8, v8, 128)
    for pack in (True, False):
        for splits in (1, 3):
            got = run_sched(q, k8, v8, cu, lens, MAXQ, bt, causal=True, splits=splits, scale=scale, pack=pack, kd=kd, vd=vd)
            assert_matches(*got, ref, what=f"fp8 scheduled paged={paged} pack={pack} splits{splits}")
            want = V.run(q, k8, v8, cu, lens, MAXQ, bt, causal=True, splits=splits, scale=scale, pack=pack, kd=kd, vd=vd)
            assert_same_bits(got, want, ref[2], f"fp8 paged={paged} pack={pack} splits{splits}")


# ---- 3. against fp64 ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page", [0, 128])
@pytest.mark.parametrize("causal", [True, False])
def test_against_fp64(page, causal):
    dtype, D = torch.bfloat16, 64
    scale = 1.0 / math.sqrt(D)
    for name, nq, lens_l, max_q in (("ragged", NQ, LENS, MAXQ), ("odd", ODD_NQ, ODD_LENS, ODD_MAXQ)):
        gen = torch.Generator().manual_seed(1300 + page)
        q, kc, vc, cu, lens = batch(gen, dtype, D, nq, lens_l)
        bt = None
        if page:
            kc, vc, bt = make_paged(gen, kc, vc, page)
        ref = reference(q, kc, vc, cu, lens, bt, scale, causal, max_q)
        assert ref[2].all()
        if causal and name == "ragged":                 # len 3 < nq 5: the first two rows see nothing; len 0: none does
            assert torch.isinf(ref[1][:, 50:52]).all() and torch.isfinite(ref[1][:, 52:55]).all() and torch.isinf(ref[1][:, 49]).all()
        for splits in (1, 3):
            out, lse = run_sched(q, kc, vc, cu, lens, max_q, bt, causal=causal, splits=splits, scale=scale)
            assert_matches(out, lse, ref, what=f"scheduled {name} page{page} causal={causal} splits{splits}")


@pytest.mark.parametrize("heads", [(8, 8), (8, 1), (6, 2)])
def test_mha_and_unpacked(heads):
    """H == Hk (MHA: the unpacked scheduled units), MQA and G = 3; pack_gqa False runs the unpacked units at every group size."""
    gen = torch.Generator().manual_seed(1400 + heads[0] * 10 + heads[1])
    dtype, D = torch.bfloat16, 64
    q, kc, vc, cu, lens = batch(gen, dtype, D, NQ, LENS, heads=heads)
    scale = 1.0 / math.sqrt(D)
    ref = reference(q, kc, vc, cu, lens, None, scale, True, MAXQ)
    for pack in (True, False):
        md = metadata(cu, MAXQ, q.shape[0], heads, causal=True, pack=pack).cpu()
        assert md[2].item() == (heads[0] // heads[1] if pack and heads[0] > heads[1] else 1)
        for splits in (1, 2):
            got = run_sched(q, kc, vc, cu, lens, MAXQ, causal=True, splits=splits, scale=scale, pack=pack)
            assert_matches(*got, ref, what=f"scheduled H{heads[0]} Hk{heads[1]} pack={pack} splits{splits}")
            want = V.run(q, kc, vc, cu, lens, MAXQ, causal=True, splits=splits, scale=scale, pack=pack)
            assert_same_bits(got, want, ref[2], f"H{heads[0]} Hk{heads[1]} pack={pack} splits{splits}")


# ---- 4 / 5. the C ABI over tensors carved out of larger allocations ---------------------------------------------------------------------------------------
class Carved(V.Carved):
    """tests/test_kvcache_varlenq_gpu.py's carved tensors, through tfa_fwd_kvcache_varlen_sched; meta: an int32 device tensor, or None = the batch's own list,
    built by tfa_kvcache_varlen_schedule into a buffer with guard words around it."""

    def call_sched(self, kc, vc, cu, lens, max_q, bt, causal, splits, scale, pack=_lib.TFA_PACK_GQA_AUTO, meta=None):
        L = _lib.lib()
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
        p.softmax_scale, p.is_causal, p.dtype = float(scale), 1 if causal else 0, V.ops._DT[self.q.dtype]
        vq = _lib.TfaKvcacheVarlenQ()
        vq.cu_seqlens_q, vq.max_seqlen_q, vq.total_q = cu.data_ptr(), max_q, self.total_q
        size = L.tfa_kvcache_varlen_schedule_size(C.byref(p), C.byref(vq), pack, p.is_causal)
        assert size > 0
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        with torch.cuda.device(self.q.device):
            if meta is None:
                whole = torch.full((16 + size + 16,), -77, dtype=torch.int32, device=DEV)
                meta = whole[16:16 + size]
                _lib.check(L.tfa_kvcache_varlen_schedule(C.byref(p), C.byref(vq), pack, p.is_causal, C.c_void_p(meta.data_ptr()), stream))
                torch.cuda.synchronize()
                assert (whole[:16] == -77).all() and (whole[16 + size:] == -77).all(), "a guard band around the metadata was overwritten"
            assert meta.numel() == size and meta.dtype == torch.int32 and meta.is_contiguous()
            need = L.tfa_fwd_kvcache_varlen_workspace(C.byref(p), C.byref(vq), None, pack, splits)
            assert need == self.ws_floats, (need, self.ws_floats)
            ws = self.ws_whole[64:].data_ptr() if self.ws_whole is not None else None
            _lib.check(L.tfa_fwd_kvcache_varlen_sched(C.byref(p), C.byref(vq), None, pack, splits, C.c_void_p(meta.data_ptr()), ws, stream))
        torch.cuda.synchronize()


@pytest.mark.parametrize("paged", [False, True])
def test_nothing_leaks_in_or_out(paged):
    """NaN behind every length, in unreferenced pages and in the q rows outside every sequence (two in front of cu[0], three behind cu[B])."""
    gen = torch.Generator().manual_seed(1500)
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
        out, lse = run_sched(q, kc, vc, cu, lens, MAXQ, bt, causal=True, splits=splits, scale=scale)
        assert_matches(out, lse, ref, what=f"scheduled, NaN around, paged={paged} splits{splits}")
    kc_d, vc_d, cu_d, lens_d = kc.to(DEV), vc.to(DEV), cu.to(DEV), lens.to(DEV)
    bt_d = None if bt is None else bt.to(DEV)
    c = Carved(q, dense_out=False)                      # one chunk: out laid out like q
    c.call_sched(kc_d, vc_d, cu_d, lens_d, MAXQ, bt_d, True, 1, scale)
    assert_matches(c.out, c.lse, ref, what=f"scheduled C ABI splits1 paged={paged}")
    c.check_untouched(ref[2])
    c = Carved(q, dense_out=True, ws_floats=3 * H * total_q * (D + 1))
    c.call_sched(kc_d, vc_d, cu_d, lens_d, MAXQ, bt_d, True, 3, scale)
    assert_matches(c.out, c.lse, ref, what=f"scheduled C ABI splits3 paged={paged}")
    c.check_untouched(torch.ones(total_q, dtype=torch.bool))      # (the merge writes every row of the dense out: the bands only)


@pytest.mark.parametrize("pack", [_lib.TFA_PACK_GQA_ON, _lib.TFA_PACK_GQA_OFF])
@pytest.mark.parametrize("causal", [True, False])
def test_clamping(pack, causal):
    """Lists that do not belong to the batch (tests/kvcache_sched_ref.py: foreign_lists — built for other row counts, n_items far above the bound, negative and huge
    (b, wi), duplicated rows, random words; tests/test_kvcache_sched_abi.py runs them through the restated decode first): the kernel clamps and verifies every
    entry, so no store lands outside the rows the batch owns — the bands around out, lse and the workspace and the rows of no sequence keep their canaries.  The
    owned rows are unspecified.  The batch's own list, through the same carved tensors, gives the reference; so does a cu_seqlens_q with out-of-range entries."""
    gen = torch.Generator().manual_seed(1600)
    dtype, D, cap = torch.float16, 64, 512
    gp = H // HK if pack == _lib.TFA_PACK_GQA_ON else 1
    scale = 1.0 / math.sqrt(D)
    cu, lens, total_q = torch.tensor(R.CLAMP_CU, dtype=torch.int32), torch.tensor(LENS, dtype=torch.int32), R.CLAMP_TOTAL_Q
    assert R.CLAMP_NQ == NQ and R.CLAMP_MAXQ == MAXQ and torch.equal(cu, cu_of(NQ, start=2))
    q = randn(gen, total_q, H, D, dtype=dtype, std=1.0)
    kc, vc = randn(gen, len(NQ), cap, HK, D, dtype=dtype), randn(gen, len(NQ), cap, HK, D, dtype=dtype)
    ref = reference(q, kc, vc, cu, lens, None, scale, causal, MAXQ)
    kc_d, vc_d, cu_d, lens_d = kc.to(DEV), vc.to(DEV), cu.to(DEV), lens.to(DEV)
    c = Carved(q, dense_out=False)
    c.call_sched(kc_d, vc_d, cu_d, lens_d, MAXQ, None, causal, 1, scale, pack)
    assert_matches(c.out, c.lse, ref, what=f"own list pack={pack} causal={causal}")
    c.check_untouched(ref[2])
    lists = R.foreign_lists(R.CLAMP_CU, MAXQ, total_q, gp, causal, R.CLAMP_OTHER_NQ)
    for name, words in lists.items():
        R.decode(words, cu.tolist(), MAXQ, total_q, gp, causal)              # (asserts in-range blocks: the CPU test's check, on exactly these words)
        meta = torch.tensor(words, dtype=torch.int32).to(DEV)
        c = Carved(q, dense_out=False)
        c.call_sched(kc_d, vc_d, cu_d, lens_d, MAXQ, None, causal, 1, scale, pack, meta=meta)
        c.check_untouched(ref[2])
        assert torch.equal(meta.cpu(), torch.tensor(words, dtype=torch.int32)), f"{name}: the attention call wrote to the metadata"
        if name == "duplicated rows":                   # split: the partials of foreign items stay inside the workspace
            c = Carved(q, dense_out=True, ws_floats=3 * H * total_q * (D + 1))
            c.call_sched(kc_d, vc_d, cu_d, lens_d, MAXQ, None, causal, 3, scale, pack, meta=meta)
            c.check_untouched(torch.ones(total_q, dtype=torch.bool))
    # V.test_clamping's batch: a cu_seqlens_q whose last entry exceeds total_q and an nq_b above max_seqlen_q — schedule and attention clamp alike
    total_q, max_q = 20, 8
    cu = torch.tensor([0, 5, 17, 30], dtype=torch.int32)
    lens = torch.tensor([100, 200, 64], dtype=torch.int32)
    q = randn(gen, total_q, H, D, dtype=dtype, std=1.0)
    kc, vc = randn(gen, 3, 256, HK, D, dtype=dtype), randn(gen, 3, 256, HK, D, dtype=dtype)
    ref = reference(q, kc, vc, cu, lens, None, scale, causal, max_q)
    assert ref[2].tolist() == [True] * 13 + [False] * 4 + [True] * 3
    c = Carved(q, dense_out=False)
    c.call_sched(kc.to(DEV), vc.to(DEV), cu.to(DEV), lens.to(DEV), max_q, None, causal, 1, scale, pack)
    assert_matches(c.out, c.lse, ref, what=f"clamped cu_seqlens_q pack={pack} causal={causal}")
    c.check_untouched(ref[2])


# ---- 6. a captured step: schedule + attention ---------------------------------------------------------------------------------------------------------------
def test_captured_step_follows_in_place_updates():
    """The list and the attention call captured in one graph; cu_seqlens_q and cache_seqlens overwritten in place (the same total_q and max_seqlen_q): every replay
    equals a fresh eager call on the new arrays, bit for bit — the list is rebuilt by the replay, the grid (sized by the host-known bound) is the same."""
    gen = torch.Generator().manual_seed(1700)
    dtype, D, cap, B, total_q, max_q = torch.bfloat16, 64, 512, 4, 60, 40
    steps = [([1, 40, 1, 18], [100, 300, 0, 64]), ([20, 0, 40, 0], [17, 129, 200, 5]), ([15, 15, 15, 15], [0, 63, 250, 496]), ([1, 1, 25, 33], [512, 1, 77, 33])]
    kc, vc = randn(gen, B, cap, HK, D, dtype=dtype).to(DEV), randn(gen, B, cap, HK, D, dtype=dtype).to(DEV)
    q = randn(gen, total_q, H, D, dtype=dtype, std=1.0).to(DEV)
    cu_dev, lens_dev = cu_of(steps[0][0]).to(DEV), torch.tensor(steps[0][1], dtype=torch.int32, device=DEV)
    md_buf = torch.zeros(R.HDR + 2 * R.bound_of(B, max_q, total_q, H // HK, True), dtype=torch.int32, device=DEV)

    def step(md_out):
        md = tfa.get_scheduler_metadata(cu_dev, max_q, total_q, H, HK, causal=True, out=md_out)
        res = [tfa.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens_dev, causal=True, num_splits=s, return_softmax_lse=True, cu_seqlens_q=cu_dev,
                                           max_seqlen_q=max_q, scheduler_metadata=md) for s in (1, 2)]      # two layers of the step share the list
        return res, md

    with torch.no_grad():
        step(None)                                       # warm-up outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            res_s, md_s = step(md_buf)
        assert md_s is md_buf
        for r, (nq, lens) in enumerate(steps):
            assert sum(nq) == total_q and max(nq) <= max_q
            cu_dev.copy_(cu_of(nq).to(DEV))
            lens_dev.copy_(torch.tensor(lens, dtype=torch.int32, device=DEV))
            q.copy_(randn(gen, total_q, H, D, dtype=dtype, std=1.0).to(DEV))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            want = R.schedule(cu_of(nq).tolist(), max_q, total_q, H // HK, True)
            assert md_buf[:len(want)].tolist() == want, f"replay {r}: the list was not rebuilt from the new cu_seqlens_q"
            res_r = [(o.clone(), l.clone()) for o, l in res_s]
            res_e, _ = step(None)                        # the eager step on the new values
            torch.cuda.synchronize()
            for (o_r, l_r), (o_e, l_e) in zip(res_r, res_e):
                assert torch.equal(o_r, o_e) and torch.equal(l_r, l_e), f"replay {r} differs from the eager step in bits"
                assert torch.isfinite(l_r).any() and not torch.isnan(o_r).any()
            ref = reference(q.cpu(), kc.cpu(), vc.cpu(), cu_of(nq), torch.tensor(lens, dtype=torch.int32), None, 1.0 / math.sqrt(D), True, max_q)
            assert_matches(*res_r[0], ref, what=f"replay {r}")
