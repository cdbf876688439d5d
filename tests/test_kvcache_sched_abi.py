"""CPU tests of the scheduled packed-q K/V-cache call (include/tfa.h: tfa_kvcache_varlen_schedule, _schedule_size, _schedule_plan, tfa_fwd_kvcache_varlen_sched,
_sched_plan) and of ``get_scheduler_metadata`` / ``flash_attn_with_kvcache(scheduler_metadata=)``: sizes, plans and refusal codes, the bound proven by
enumeration, the kernel's decode of a list entry (restated, clamps included) over the lists the GPU clamping test feeds it, and the wrapper's calls and refusals
against a counting stand-in for the library.  No GPU: plans never launch, refused calls return before any launch."""
import ctypes as C
import itertools

import pytest
import torch

import kvcache_sched_ref as R
import test_kvcache_varlenq_abi as VA
import tiny_flash_attention_amd as tfa
from tiny_flash_attention_amd import _lib, ops

ADDR, CODES, AUTO, ON, OFF = VA.ADDR, VA.CODES, VA.AUTO, VA.ON, VA.OFF
params, varlen = VA.params, VA.varlen
SCHED_SYMBOLS = ("tfa_kvcache_varlen_schedule_size", "tfa_kvcache_varlen_schedule", "tfa_kvcache_varlen_schedule_plan", "tfa_fwd_kvcache_varlen_sched",
                 "tfa_fwd_kvcache_varlen_sched_plan")
# the GPU tests' ragged batch (tests/test_kvcache_varlenq_gpu.py) and the rows of another batch of the same size
NQ, MAXQ = [1, 0, 7, 1, 40, 1, 5], 40
OTHER_NQ = [40, 1, 0, 0, 2, 7, 5]
ODD_NQ, ODD_MAXQ = [2, 70, 0, 3], 70          # 70 * 4 = 280 packed rows: three blocks, the middle one alone under causal


def cu_of(nq, start=0):
    c = [start]
    for n in nq:
        c.append(c[-1] + n)
    return c


def size(p, vq, mode=AUTO, causal=0):
    return _lib.lib().tfa_kvcache_varlen_schedule_size(C.byref(p) if p is not None else None, C.byref(vq) if vq is not None else None, mode, causal)


def schedule_plan(p, vq, mode=AUTO, causal=0):
    g, b, l = C.c_int(), C.c_int(), C.c_int()
    st = _lib.lib().tfa_kvcache_varlen_schedule_plan(C.byref(p) if p is not None else None, C.byref(vq) if vq is not None else None, mode, causal,
                                                     C.byref(g), C.byref(b), C.byref(l))
    return st, g.value, b.value, l.value


def sched_plan(p, vq, mode=AUTO, splits=1, q8=None):
    g, b, l = C.c_int(), C.c_int(), C.c_int()
    st = _lib.lib().tfa_fwd_kvcache_varlen_sched_plan(C.byref(p) if p is not None else None, C.byref(vq) if vq is not None else None,
                                                      C.byref(q8) if q8 is not None else None, mode, splits, C.byref(g), C.byref(b), C.byref(l))
    return st, g.value, b.value, l.value


def test_symbols_exported():
    L = _lib.lib()
    for s in SCHED_SYMBOLS:
        assert s in _lib.SYMBOLS
        getattr(L, s)
    assert tfa.get_scheduler_metadata is ops.get_scheduler_metadata and "get_scheduler_metadata" in tfa.__all__


def test_schedule_size_and_plan():
    """8 header words + 2 per item row; the bound as the header states it; of *p only B, H, Hk are read."""
    for B, H, Hk, mq, tq in ((7, 8, 2, 40, 55), (64, 32, 8, 512, 60 + 4 * 512), (256, 32, 8, 2048, 255 + 2048), (3, 8, 8, 5, 9), (2, 256, 1, 3, 6), (5, 16, 1, 1, 5)):
        G = H // Hk
        packs = Hk < H and G <= 128
        for causal in (0, 1):
            p, vq = params(B=B, H=H, Hk=Hk, total_q=tq), varlen(mq, tq)
            bare = _lib.TfaKvcacheParams()
            bare.B, bare.H, bare.Hk = B, H, Hk
            for mode, gp in ((AUTO, G if packs else 1), (ON, G if packs else 1), (OFF, 1)):
                want = R.HDR + 2 * R.bound_of(B, mq, tq, gp, bool(causal))
                assert size(p, vq, mode, causal) == size(bare, vq, mode, causal) == want
                assert schedule_plan(p, vq, mode, causal) == (0, 1, 256, 256 * 8)
    # hand-computed: B 64, H32 Hk8 packed, max_seqlen_q 512 (16 blocks), total_q 2108: F = ceil(2108 * 4 / 128) = 66
    p, vq = params(B=64, H=32, Hk=8, total_q=2108), varlen(512, 2108)
    assert size(p, vq, ON, 0) == 8 + 2 * min(64 * 16, 66 + 64) == 8 + 2 * 130
    assert size(p, vq, ON, 1) == 8 + 2 * min(64 * 8, (66 + 128) // 2) == 8 + 2 * 97
    assert size(p, vq, OFF, 0) == 8 + 2 * min(64 * 4, 17 + 64)


def test_schedule_refusals():
    L = _lib.lib()
    p, vq = params(), varlen()
    assert size(None, vq) == size(p, None) == CODES["TFA_ERR_NULL"]
    assert schedule_plan(None, vq)[0] == schedule_plan(p, None)[0] == CODES["TFA_ERR_NULL"]
    v = varlen()
    v.cu_seqlens_q = None
    assert schedule_plan(p, v)[0] == CODES["TFA_ERR_NULL"]
    assert L.tfa_kvcache_varlen_schedule(C.byref(p), C.byref(vq), ON, 0, None, None) == CODES["TFA_ERR_NULL"]
    assert L.tfa_kvcache_varlen_schedule(C.byref(p), C.byref(vq), ON, 0, ADDR + 4, None) == CODES["TFA_ERR_ALIGN"]      # 8-byte rows
    for off in (1, 2):
        v = varlen()
        v.cu_seqlens_q = ADDR + off
        assert schedule_plan(p, v)[0] == CODES["TFA_ERR_ALIGN"]
    for kw in (dict(max_q=0), dict(max_q=-3), dict(total_q=0), dict(total_q=-1)):
        v = varlen(**{**dict(max_q=16, total_q=64), **kw})
        assert size(p, v) == schedule_plan(p, v)[0] == CODES["TFA_ERR_SHAPE"]
    for i in (0, 1):
        v = varlen()
        v.reserved_[i] = 1
        assert size(p, v) == schedule_plan(p, v)[0] == CODES["TFA_ERR_SHAPE"]
    for kw in (dict(B=0), dict(Hk=0), dict(H=12, Hk=8), dict(H=0)):
        assert size(params(**kw), vq) == schedule_plan(params(**kw), vq)[0] == CODES["TFA_ERR_SHAPE"]
    for mode in (3, -1, 1 << 20):
        assert size(p, vq, mode) == schedule_plan(p, vq, mode)[0] == CODES["TFA_ERR_SHAPE"]
        assert L.tfa_kvcache_varlen_schedule(C.byref(p), C.byref(vq), mode, 0, ADDR, None) == CODES["TFA_ERR_SHAPE"]


@pytest.mark.parametrize("splits", [1, 2, 8])
@pytest.mark.parametrize("causal", [False, True])
def test_sched_plan_grid_is_heads_times_bound_times_chunks(splits, causal):
    for B, H, Hk, D, mq, tq in ((7, 8, 2, 64, 40, 55), (3, 16, 4, 128, 33, 50), (3, 8, 8, 64, 5, 9), (64, 32, 8, 128, 512, 2108)):
        G = H // Hk
        p, vq = params(B=B, H=H, Hk=Hk, D=D, cap=1024, total_q=tq, causal=causal), varlen(mq, tq)
        gp = G if G > 1 else 1
        assert sched_plan(p, vq, ON, splits) == sched_plan(p, vq, AUTO, splits) == (0, Hk * R.bound_of(B, mq, tq, gp, causal) * splits, 256, 4 * 64 * D * 2)
        assert sched_plan(p, vq, OFF, splits) == (0, H * R.bound_of(B, mq, tq, 1, causal) * splits, 256, 4 * 64 * D * 2)
        for mode in (ON, OFF):
            assert sched_plan(p, vq, mode, splits)[1] <= VA.plan(p, vq, mode, splits)[1]
    p, vq = params(B=3, H=8, Hk=2, D=64, cap=1024, total_q=9, page=128, causal=causal), varlen(5, 9)
    q8 = _lib.TfaKvcacheFp8()
    q8.format = _lib.TFA_KV_E4M3
    assert sched_plan(p, vq, ON, splits, q8) == (0, 2 * 3 * splits, 256, 4 * 64 * 64 * 2)


def test_sched_plan_is_below_the_unscheduled_grid_on_a_mixed_batch():
    """B 64, H32 Hk8, 60 decode rows + 4 chunks of 512, packed, not causal: 8 * 130 workgroups instead of 64 * 8 * 16."""
    p, vq = params(B=64, H=32, Hk=8, D=128, cap=8192, total_q=60 + 4 * 512), varlen(512, 60 + 4 * 512)
    st, grid, _, _ = sched_plan(p, vq, ON)
    st0, grid0, _, _ = VA.plan(p, vq, ON)
    assert st == st0 == 0 and grid == 8 * 130 and grid0 == 64 * 8 * 16 and grid < grid0
    L = _lib.lib()
    for mode in (ON, OFF):                               # the workspace and the split suggestion are the unscheduled call's
        assert L.tfa_fwd_kvcache_varlen_workspace(C.byref(p), C.byref(vq), None, mode, 3) == 3 * 32 * (60 + 4 * 512) * 129


def test_sched_refusals():
    L = _lib.lib()
    p, vq = params(), varlen()
    call = lambda p, vq, mode, splits, meta, ws: L.tfa_fwd_kvcache_varlen_sched(C.byref(p), C.byref(vq), None, mode, splits, meta, ws, None)
    assert call(p, vq, ON, 1, None, None) == CODES["TFA_ERR_NULL"]
    assert call(p, vq, ON, 1, ADDR + 4, None) == CODES["TFA_ERR_ALIGN"]
    assert sched_plan(None, vq)[0] == sched_plan(p, None)[0] == CODES["TFA_ERR_NULL"]
    # everything tfa_fwd_kvcache_varlen_plan refuses, with its code
    cases = [(params(D=12), varlen()), (params(dtype=_lib.TFA_F32), varlen()), (params(B=0), varlen()), (params(H=12, Hk=8), varlen()), (params(), varlen(0, 64)),
             (params(), varlen(16, 0)), (params(cap=0), varlen()), (params(total_q=64, dense_out=False), varlen())]
    v = varlen()
    v.reserved_[1] = 1
    cases.append((params(), v))
    v = varlen()
    v.cu_seqlens_q = ADDR + 2
    cases.append((params(), v))
    pn = params()
    pn.n_new = 1
    cases.append((pn, varlen()))
    pq = params()
    pq.q = None
    cases.append((pq, varlen()))
    seen = set()
    for p, v in cases:
        for mode in (ON, OFF, 7):
            want = VA.plan(p, v, mode, 2)[0]
            assert want < 0 and sched_plan(p, v, mode, 2)[0] == want
            assert call(p, v, mode, 2, ADDR, ADDR) == want
            seen.add(want)
    assert len(seen) >= 5
    p, vq = params(), varlen()
    assert sched_plan(p, vq, ON, 0)[0] == CODES["TFA_ERR_SHAPE"]
    assert call(p, vq, ON, 4, ADDR, None) == CODES["TFA_ERR_NULL"] and call(p, vq, ON, 4, ADDR, ADDR + 4) == CODES["TFA_ERR_ALIGN"]      # the workspace
    # a packing the unscheduled call would silently drop (a head group's rows beyond one descriptor): the list was sized for the packing named
    big = params(B=1, H=8, Hk=2, D=128, total_q=8)
    big.q_stride[1] = 1 << 29
    assert VA.plan(big, varlen(4, 8), ON)[0] == 0 == VA.plan(big, varlen(4, 8), OFF)[0]
    assert sched_plan(big, varlen(4, 8), ON)[0] == CODES["TFA_ERR_STRIDE"] and sched_plan(big, varlen(4, 8), OFF)[0] == 0


@pytest.mark.parametrize("gp,values", [(4, (0, 1, 31, 32, 33, 64)), (1, (0, 1, 127, 128, 129))])
def test_the_bound_holds_for_every_small_batch(gp, values):
    """Every nq vector with B <= 4 over row counts that straddle block edges, causal and not, at the tightest total_q and max_seqlen_q and at looser ones: the
    items of the batch never outnumber the bound tfa_kvcache_varlen_schedule_size states (and the restated bound is the library's)."""
    H, Hk = (8, 2) if gp == 4 else (8, 8)
    checked = 0
    for B in (1, 2, 3, 4):
        p = params(B=B, H=H, Hk=Hk)
        for nq in itertools.product(values, repeat=B):
            if sum(nq) == 0:
                continue
            for causal in (False, True):
                true_items = sum(R.items_of(R.blocks_of(n, gp), causal) for n in nq)
                for tq, mq in ((sum(nq), max(nq)), (sum(nq) + 5, max(nq) + 70)):
                    bound = R.bound_of(B, mq, tq, gp, causal)
                    assert true_items <= bound, (nq, causal, tq, mq, true_items, bound)
                    if B <= 2 or checked % 37 == 0:
                        assert size(p, varlen(mq, tq), ON, int(causal)) == R.HDR + 2 * bound
                    meta = R.schedule(cu_of(nq), mq, tq, gp, causal)
                    assert meta[0] == true_items and len(meta) == R.HDR + 2 * true_items      # nothing was cut off
                    checked += 1
    assert checked > 1000


def test_schedule_restated_on_the_test_batches():
    """The lists the GPU tests expect, by hand: the ragged batch packed (G' = 4) has one item per sequence with rows — the 40-row sequence (160 packed rows) two
    blocks: two items, or ONE causal pair; the odd batch three blocks: three items, or two (the pair and the middle block alone)."""
    cu = cu_of(NQ)
    m = R.schedule(cu, MAXQ, 55, 4, False)
    assert m[:8] == [7, 7, 4, 0, 40, 55, min(7 * 2, 2 + 7), 0] and m[8:] == [0, 0, 2, 0, 3, 0, 4, 0, 4, 1, 5, 0, 6, 0]
    m = R.schedule(cu, MAXQ, 55, 4, True)
    assert m[:8] == [6, 7, 4, 1, 40, 55, min(7 * 1, (2 + 14) // 2), 0] and m[8:] == [0, 0, 2, 0, 3, 0, 4, 0, 5, 0, 6, 0]
    m = R.schedule(cu_of(ODD_NQ), ODD_MAXQ, 75, 4, True)
    assert m[0] == 4 and m[8:] == [0, 0, 1, 0, 1, 1, 3, 0]
    assert sorted(R.decode(m, cu_of(ODD_NQ), ODD_MAXQ, 75, 4, True)) == [(0, 0), (1, 0), (1, 1), (1, 2), (3, 0)]      # every block once: (2, 0) pair, 1 alone
    m = R.schedule(cu_of(ODD_NQ), ODD_MAXQ, 75, 4, False)
    assert m[0] == 5 and sorted(R.decode(m, cu_of(ODD_NQ), ODD_MAXQ, 75, 4, False)) == [(0, 0), (1, 0), (1, 1), (1, 2), (3, 0)]
    # out-of-range cu_seqlens_q entries are clamped as the attention kernel clamps them (tests/test_kvcache_varlenq_gpu.py::test_clamping's batch)
    m = R.schedule([0, 5, 17, 30], 8, 20, 4, False)
    assert R.rows_of([0, 5, 17, 30], 20, 8) == [(0, 5), (5, 8), (17, 3)] and m[0] == 3 and m[8:] == [0, 0, 1, 0, 2, 0]


@pytest.mark.parametrize("gp", [4, 1])
@pytest.mark.parametrize("causal", [True, False])
def test_decode_of_foreign_lists_touches_only_blocks_of_their_sequences(gp, causal):
    """The lists the GPU clamping test runs, through the restated decode first: whatever they hold, every read of the list lies inside its buffer and every
    (sequence, block) that runs is a block of that sequence (R.decode asserts both).  With the batch's own list every block runs exactly once."""
    assert R.CLAMP_CU == cu_of(R.CLAMP_NQ, start=2) and R.CLAMP_TOTAL_Q == R.CLAMP_CU[-1] + 3
    for cu, tq, nq, mq, other in ((R.CLAMP_CU, R.CLAMP_TOTAL_Q, R.CLAMP_NQ, R.CLAMP_MAXQ, R.CLAMP_OTHER_NQ),      # the GPU clamping test's batch, its very words
                                  (cu_of(NQ), sum(NQ), NQ, MAXQ, OTHER_NQ), (cu_of(ODD_NQ), sum(ODD_NQ), ODD_NQ, ODD_MAXQ, [70, 2, 3, 0])):
        want = sorted((b, mb) for b, n in enumerate(nq) for mb in range(R.blocks_of(n, gp)))
        assert sorted(R.decode(R.schedule(cu, mq, tq, gp, causal), cu, mq, tq, gp, causal)) == want
        lists = R.foreign_lists(cu, mq, tq, gp, causal, other)
        assert len(lists) >= 5
        for name, meta in lists.items():
            touched = R.decode(meta, cu, mq, tq, gp, causal)
            assert set(touched) <= set(want), name


# ---- Python: get_scheduler_metadata and flash_attn_with_kvcache(scheduler_metadata=) against a counting stand-in for the library ----------------------------
class _CountingLib(VA._CountingLib):
    SIZE = 26

    def __getattr__(self, name):
        base = super().__getattr__(name)

        def f(*a):
            r = base(*a)
            return self.SIZE if name == "tfa_kvcache_varlen_schedule_size" else r
        return f


@pytest.fixture
def stub(monkeypatch):
    fake = _CountingLib()
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    monkeypatch.setattr(ops.torch, "cuda", VA._FakeCuda)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(torch.Tensor, "data_ptr", lambda self: ADDR + 16 * (id(self) % 4096))
    return fake


_meta, _tensors = VA._meta, VA._tensors


def test_get_scheduler_metadata_calls(stub):
    cu = _meta(4, dtype=torch.int32)
    md = ops.get_scheduler_metadata(cu, 7, 10, 8, 2, causal=True)
    assert [c[0] for c in stub.calls] == ["tfa_kvcache_varlen_schedule_size", "tfa_kvcache_varlen_schedule"]
    pref, vref, mode, causal = stub.calls[0][1]
    assert (pref._obj.B, pref._obj.H, pref._obj.Hk, vref._obj.max_seqlen_q, vref._obj.total_q, mode, causal) == (3, 8, 2, 7, 10, ON, 1)
    pref, vref, mode, causal, meta, stream = stub.calls[1][1]
    assert (pref._obj.B, pref._obj.H, pref._obj.Hk, mode, causal) == (3, 8, 2, ON, 1) and meta.value == md.data_ptr()
    assert (vref._obj.cu_seqlens_q, vref._obj.max_seqlen_q, vref._obj.total_q, list(vref._obj.reserved_)) == (cu.data_ptr(), 7, 10, [0, 0])
    assert md.dtype == torch.int32 and tuple(md.shape) == (_CountingLib.SIZE,)
    stub.calls.clear()
    again = ops.get_scheduler_metadata(cu, 7, 10, 8, 2, pack_gqa=False, out=md)                  # out= reuses the buffer; False runs unpacked
    assert again is md and stub.calls[1][1][2:4] == (OFF, 0) and stub.calls[1][1][4].value == md.data_ptr()
    stub.calls.clear()
    for bad in (_meta(4, dtype=torch.int64), _meta(2, 2, dtype=torch.int32), _meta(1, dtype=torch.int32), _meta(8, dtype=torch.int32)[::2], [0, 3, 6, 10]):
        with pytest.raises(ValueError, match="cu_seqlens_q"):
            ops.get_scheduler_metadata(bad, 7, 10, 8, 2)
    for args in ((0, 10, 8, 2), (7, 0, 8, 2), (7, 10, 0, 2), (7, 10, 8, 0), (7.0, 10, 8, 2), (True, 10, 8, 2)):
        with pytest.raises(ValueError, match="positive host int"):
            ops.get_scheduler_metadata(cu, *args)
    with pytest.raises(ValueError, match="must divide"):
        ops.get_scheduler_metadata(cu, 7, 10, 8, 3)
    with pytest.raises(TypeError, match="pack_gqa"):
        ops.get_scheduler_metadata(cu, 7, 10, 8, 2, pack_gqa=1)
    assert stub.calls == []
    with pytest.raises(TypeError, match="out must be a tensor"):
        ops.get_scheduler_metadata(cu, 7, 10, 8, 2, out=[0] * 26)
    for bad in (_meta(25, dtype=torch.int32), _meta(26, dtype=torch.int64), _meta(52, dtype=torch.int32)[::2]):
        with pytest.raises(ValueError, match="out must be a contiguous int32 tensor of 26 entries"):
            ops.get_scheduler_metadata(cu, 7, 10, 8, 2, out=bad)
    assert all(c[0] == "tfa_kvcache_varlen_schedule_size" for c in stub.calls)                  # nothing was launched
    with pytest.raises(TypeError):
        ops.get_scheduler_metadata(cu, 7, 10, 8, 2, True)                                        # keyword-only


def test_wrapper_takes_the_scheduled_entry_point(stub):
    q, kc, vc, lens, cu = _tensors()
    md = _meta(_CountingLib.SIZE, dtype=torch.int32)
    out, lse = ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, causal=True, return_softmax_lse=True, cu_seqlens_q=cu, max_seqlen_q=7,
                                           scheduler_metadata=md)
    assert [c[0] for c in stub.calls] == ["tfa_kvcache_varlen_schedule_size", "tfa_fwd_kvcache_varlen_suggest_splits", "tfa_fwd_kvcache_varlen_workspace",
                                          "tfa_fwd_kvcache_varlen_sched"]
    pref, vref, mode, causal = stub.calls[0][1]
    assert (pref._obj.B, pref._obj.H, pref._obj.Hk, vref._obj.max_seqlen_q, vref._obj.total_q, mode, causal) == (3, 8, 2, 7, 10, ON, 1)
    pref, vref, q8, mode, splits, meta, ws, stream = stub.calls[3][1]
    p, v = pref._obj, vref._obj
    assert q8 is None and mode == ON and splits == 5 and ws is not None and meta.value == md.data_ptr()
    assert (p.B, p.H, p.Hk, p.D, p.capacity, p.is_causal) == (3, 8, 2, 64, 1024, 1)
    assert (v.cu_seqlens_q, v.max_seqlen_q, v.total_q) == (cu.data_ptr(), 7, 10)
    assert tuple(out.shape) == (10, 8, 64) and tuple(lse.shape) == (8, 10)
    stub.calls.clear()
    ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, num_splits=1, pack_gqa=False, cu_seqlens_q=cu, max_seqlen_q=7, scheduler_metadata=md)
    assert [c[0] for c in stub.calls] == ["tfa_kvcache_varlen_schedule_size", "tfa_fwd_kvcache_varlen_workspace", "tfa_fwd_kvcache_varlen_sched"]
    assert stub.calls[0][1][2:] == (OFF, 0) and stub.calls[-1][1][3:5] == (OFF, 1) and stub.calls[-1][1][6] is None


def test_wrapper_without_scheduler_metadata_takes_todays_path(stub):
    q, kc, vc, lens, cu = _tensors()
    ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, causal=True, cu_seqlens_q=cu, max_seqlen_q=7)
    ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, num_splits=3, cu_seqlens_q=cu, max_seqlen_q=7, scheduler_metadata=None)
    q4, kc4, lens4 = _meta(2, 4, 8, 64), _meta(2, 1024, 2, 64), _meta(2, dtype=torch.int32)
    ops.flash_attn_with_kvcache(q4, kc4, kc4, cache_seqlens=lens4, num_splits=2, scheduler_metadata=None)
    assert [c[0] for c in stub.calls] == ["tfa_fwd_kvcache_varlen_suggest_splits", "tfa_fwd_kvcache_varlen_workspace", "tfa_fwd_kvcache_varlen",
                                          "tfa_fwd_kvcache_varlen_workspace", "tfa_fwd_kvcache_varlen", "tfa_fwd_kvcache_workspace", "tfa_fwd_kvcache"]


def test_wrapper_refusals_of_scheduler_metadata(stub):
    q, kc, vc, lens, cu = _tensors()
    md = _meta(_CountingLib.SIZE, dtype=torch.int32)
    ok = dict(cache_seqlens=lens, cu_seqlens_q=cu, max_seqlen_q=7)
    call = lambda *a, **kw: ops.flash_attn_with_kvcache(*a, **kw)
    with pytest.raises(ValueError, match="scheduler_metadata belongs to cu_seqlens_q"):
        call(_meta(3, 4, 8, 64), kc, vc, cache_seqlens=lens, scheduler_metadata=md)
    for bad in ([0] * 26, 26, "md"):
        with pytest.raises(TypeError, match="scheduler_metadata must be the tensor"):
            call(q, kc, vc, scheduler_metadata=bad, **ok)
    with pytest.raises(ValueError, match="contiguous int32 tensor on q's device"):
        call(q, kc, vc, scheduler_metadata=_meta(26, dtype=torch.int64), **ok)
    with pytest.raises(ValueError, match="contiguous int32 tensor on q's device"):
        call(q, kc, vc, scheduler_metadata=_meta(52, dtype=torch.int32)[::2], **ok)
    with pytest.raises(ValueError, match="contiguous int32 tensor on q's device"):
        call(q, kc, vc, scheduler_metadata=torch.zeros(26, dtype=torch.int32), **ok)
    assert stub.calls == []
    for n in (25, 27, 8):
        with pytest.raises(ValueError, match="built for another batch"):
            call(q, kc, vc, scheduler_metadata=_meta(n, dtype=torch.int32), **ok)
    assert all(c[0] == "tfa_kvcache_varlen_schedule_size" for c in stub.calls)                  # a host computation: nothing was launched
    stub.calls.clear()
    # everything the packed-q call refuses stays refused with today's messages
    with pytest.raises(NotImplementedError, match="softcap"):
        call(q, kc, vc, softcap=30.0, scheduler_metadata=md, **ok)
    with pytest.raises(NotImplementedError, match="window_size"):
        call(q, kc, vc, window_size=(128, 0), scheduler_metadata=md, **ok)
    with pytest.raises(NotImplementedError, match="cache_leftpad"):
        call(q, kc, vc, cache_leftpad=lens, scheduler_metadata=md, **ok)
    with pytest.raises(ValueError, match="kvcache_append_varlen"):
        call(q, kc, vc, _meta(10, 2, 64), _meta(10, 2, 64), scheduler_metadata=md, **ok)
    with pytest.raises(ValueError, match="max_seqlen_q"):
        call(q, kc, vc, cache_seqlens=lens, cu_seqlens_q=cu, scheduler_metadata=md)
    with pytest.raises(TypeError):
        ops.flash_attn_with_kvcache(q, kc, vc, None, None, lens, None, None, False, 0, False, md)      # keyword-only
    assert stub.calls == []
