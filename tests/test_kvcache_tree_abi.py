"""CPU tests of the tree mask over a K/V cache (include/tfa.h: tfa_fwd_kvcache_tree, _tree_plan, _tree_workspace, _tree_suggest_splits) and of
``flash_attn_with_kvcache(tree_mask=)``: the symbols, plans (the underlying form's grid), refusal codes, the split suggestion, the bool -> int64 packing, and the
wrapper's calls and refusals against a counting stand-in for the library.  No GPU: plans never launch, refused calls return before any launch."""
import ctypes as C
import inspect

import pytest
import torch
import torch._dynamo.utils  # noqa: F401  (the meta kernels of the bool packing load it lazily and it reads torch.cuda: in front of the stand-in below)

import test_kvcache_sched_abi as SA
import test_kvcache_varlenq_abi as VA
import test_kvcache_window_abi as WA
from tiny_flash_attention_amd import _lib, ops

ADDR, CODES, AUTO, ON, OFF = VA.ADDR, VA.CODES, VA.AUTO, VA.ON, VA.OFF
TREE_SYMBOLS = ("tfa_fwd_kvcache_tree", "tfa_fwd_kvcache_tree_plan", "tfa_fwd_kvcache_tree_workspace", "tfa_fwd_kvcache_tree_suggest_splits")
_meta, params4, ref, pack_plan = VA._meta, WA.params4, WA.ref, WA.pack_plan


def tree(mask=ADDR, bs=5, rs=1):
    t = _lib.TfaKvcacheTree()
    t.mask, t.batch_stride, t.row_stride = mask, bs, rs
    return t


def tplan(p, vq, tr, mode=AUTO, splits=1, q8=None, scheduled=0):
    g, b, l = C.c_int(), C.c_int(), C.c_int()
    st = _lib.lib().tfa_fwd_kvcache_tree_plan(ref(p), ref(vq), ref(q8), mode, ref(tr), splits, scheduled, C.byref(g), C.byref(b), C.byref(l))
    return st, g.value, b.value, l.value


def test_symbols_exported_version_and_signature():
    L = _lib.lib()
    for s in TREE_SYMBOLS:
        assert s in _lib.SYMBOLS
        getattr(L, s)
    assert L.tfa_version() == 111
    names = list(inspect.signature(ops.flash_attn_with_kvcache).parameters)
    assert names[names.index("tree_mask") + 1] == "scheduler_metadata" and names[-3:] == ["sliding_window", "k_descale", "v_descale"]
    par = inspect.signature(ops.flash_attn_with_kvcache).parameters["tree_mask"]
    assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is None
    assert C.sizeof(_lib.TfaKvcacheTree) == 24 and [f[0] for f in _lib.TfaKvcacheTree._fields_] == ["mask", "batch_stride", "row_stride"]


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splits", [1, 3])
def test_tree_plan_grid_is_the_underlying_forms(splits):
    fp8 = _lib.TfaKvcacheFp8()
    fp8.format = _lib.TFA_KV_E4M3
    tr = tree()
    for q8 in (None, fp8):
        # 4-D, several rows: tfa_fwd_kvcache_pack_plan's
        for Nq, page in ((5, 0), (64, 128), (33, 0)):
            p = params4(Nq=Nq, page=page)
            for mode in (AUTO, ON, OFF):
                want = pack_plan(p, mode, splits, q8)
                assert want[0] == 0 and tplan(p, None, tr, mode, splits, q8) == want
        # 4-D, one row: AUTO and ON run position-major packed rows (one workgroup per (b, hk, chunk)), OFF one per query head — the plain call's grids
        p = params4(Nq=1)
        assert tplan(p, None, tr, AUTO, splits, q8) == tplan(p, None, tr, ON, splits, q8) == (0, 3 * 2 * splits, 256, 4 * 64 * 64 * 2) == pack_plan(p, AUTO, splits, q8)
        assert tplan(p, None, tr, OFF, splits, q8) == (0, 3 * 8 * splits, 256, 4 * 64 * 64 * 2) == pack_plan(p, OFF, splits, q8)
        # packed q, unscheduled and scheduled
        for mq, tq in ((5, 9), (40, 50)):
            p, vq = VA.params(B=3, H=8, Hk=2, D=64, cap=1024, total_q=tq, causal=True), VA.varlen(mq, tq)
            for mode in (AUTO, ON, OFF):
                assert tplan(p, vq, tr, mode, splits, q8) == VA.plan(p, vq, mode, splits, q8) and VA.plan(p, vq, mode, splits, q8)[0] == 0
                assert tplan(p, vq, tr, mode, splits, q8, scheduled=1) == SA.sched_plan(p, vq, mode, splits, q8)


def test_tree_plan_refusals():
    L = _lib.lib()
    p, pv, vq, tr = params4(), VA.params(total_q=64, causal=True), VA.varlen(), tree()
    assert tplan(None, None, tr)[0] == tplan(None, vq, tr)[0] == CODES["TFA_ERR_NULL"]
    assert tplan(p, None, None)[0] == tplan(pv, vq, None)[0] == tplan(p, None, tree(mask=None))[0] == CODES["TFA_ERR_NULL"]
    assert tplan(p, None, tree(mask=ADDR + 4))[0] == tplan(pv, vq, tree(mask=ADDR + 4))[0] == CODES["TFA_ERR_ALIGN"]
    assert tplan(p, None, tree(rs=-1))[0] == tplan(p, None, tree(bs=-1))[0] == tplan(pv, vq, tree(rs=-1))[0] == CODES["TFA_ERR_STRIDE"]
    assert tplan(pv, vq, tree(bs=-1))[0] == 0                                             # the batch stride is not read in the packed form
    assert tplan(p, None, tree(bs=0, rs=0))[0] == 0                                         # a broadcast word
    assert tplan(params4(causal=False), None, tr)[0] == tplan(VA.params(total_q=64, causal=False), vq, tr)[0] == CODES["TFA_ERR_SHAPE"]
    assert tplan(p, None, tr, scheduled=1)[0] == CODES["TFA_ERR_SHAPE"]                     # a list without cu_seqlens_q
    assert L.tfa_fwd_kvcache_tree(C.byref(p), None, None, AUTO, C.byref(tr), 1, ADDR, None, None) == CODES["TFA_ERR_SHAPE"]
    assert L.tfa_fwd_kvcache_tree(C.byref(p), None, None, AUTO, None, 1, None, None, None) == CODES["TFA_ERR_NULL"]
    assert L.tfa_fwd_kvcache_tree(C.byref(pv), C.byref(vq), None, ON, C.byref(tr), 1, ADDR + 4, None, None) == CODES["TFA_ERR_ALIGN"]      # the scheduled form's own check
    # every other check is the underlying form's, with its code
    seen = set()
    for bad in (params4(D=12), params4(dtype=_lib.TFA_F32), params4(B=0), params4(H=12, Hk=8), params4(cap=0), params4(Nq=0)):
        for mode in (AUTO, ON, OFF, 7):
            want = pack_plan(bad, mode, 2)[0]
            assert want < 0 and tplan(bad, None, tr, mode, 2)[0] == want
            seen.add(want)
    for bad, v in ((VA.params(D=12, causal=True), vq), (VA.params(causal=True), VA.varlen(0, 64)), (VA.params(causal=True), VA.varlen(16, 0)),
                   (VA.params(total_q=64, dense_out=False, causal=True), vq)):
        want = VA.plan(bad, v, ON, 2)[0]
        assert want < 0 and tplan(bad, v, tr, ON, 2)[0] == want and tplan(bad, v, tr, ON, 2, scheduled=1)[0] == want
        seen.add(want)
    assert len(seen) >= 4
    assert tplan(p, None, tr, AUTO, 0)[0] == CODES["TFA_ERR_SHAPE"]


def test_tree_workspace_and_split_suggestion_are_the_underlying_forms():
    L = _lib.lib()
    tr = tree()
    p = params4(Nq=5)
    pv, vq = VA.params(B=3, H=8, Hk=2, D=64, cap=1024, total_q=9, causal=True), VA.varlen(5, 9)
    for mode in (AUTO, ON, OFF):
        for splits in (1, 2, 5, 64):
            assert L.tfa_fwd_kvcache_tree_workspace(C.byref(p), None, None, mode, C.byref(tr), splits) == L.tfa_fwd_kvcache_pack_workspace(C.byref(p), None, mode, splits)
            assert (L.tfa_fwd_kvcache_tree_workspace(C.byref(pv), C.byref(vq), None, mode, C.byref(tr), splits)
                    == L.tfa_fwd_kvcache_varlen_workspace(C.byref(pv), C.byref(vq), None, mode, splits))
    assert L.tfa_fwd_kvcache_tree_workspace(C.byref(p), None, None, AUTO, C.byref(tr), 2) == 2 * 3 * 8 * 5 * 65
    assert L.tfa_fwd_kvcache_tree_workspace(C.byref(p), None, None, AUTO, None, 2) == CODES["TFA_ERR_NULL"]
    for Nq in (1, 8, 64):
        big = params4(B=1, H=32, Hk=8, D=128, cap=16384, Nq=Nq)
        for mode in (AUTO, ON, OFF):
            assert L.tfa_fwd_kvcache_tree_suggest_splits(C.byref(big), None, mode, C.byref(tr)) == L.tfa_fwd_kvcache_pack_suggest_splits(C.byref(big), mode)
    bv, bq = VA.params(B=1, H=32, Hk=8, cap=16384, total_q=8, causal=True), VA.varlen(8, 8)
    assert L.tfa_fwd_kvcache_tree_suggest_splits(C.byref(bv), C.byref(bq), ON, C.byref(tr)) == L.tfa_fwd_kvcache_varlen_suggest_splits(C.byref(bv), C.byref(bq), ON) > 1
    assert L.tfa_fwd_kvcache_tree_suggest_splits(None, None, AUTO, None) == 1


# ---- Python: flash_attn_with_kvcache(tree_mask=) against a counting stand-in for the library -----------------------------------------------------------------
class _CountingLib(SA._CountingLib):
    def __getattr__(self, name):
        base = super().__getattr__(name)

        def f(*a):
            r = base(*a)
            if name == "tfa_fwd_kvcache_tree_suggest_splits":
                return 3
            if name == "tfa_fwd_kvcache_tree_workspace":
                p, vq, s = a[0]._obj, a[1], a[-1]
                rows = p.H * vq._obj.total_q if vq is not None else p.B * p.H * p.Nq
                return s * rows * (p.D + 1) if s > 1 else 0
            return r
        return f


@pytest.fixture
def stub(monkeypatch):
    fake = _CountingLib()
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    monkeypatch.setattr(ops.torch, "cuda", VA._FakeCuda)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(torch.Tensor, "data_ptr", lambda self: ADDR + 16 * (id(self) % 4096))
    return fake


TREE_CALLS = ["tfa_fwd_kvcache_tree_suggest_splits", "tfa_fwd_kvcache_tree_workspace", "tfa_fwd_kvcache_tree"]
_t4 = WA._t4


def test_without_tree_mask_the_calls_are_todays(stub):
    q, kc, vc, lens, cu = VA._tensors()
    ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, causal=True, cu_seqlens_q=cu, max_seqlen_q=7)
    ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, num_splits=3, cu_seqlens_q=cu, max_seqlen_q=7, tree_mask=None)
    q4, kc4, vc4, lens4 = _t4()
    ops.flash_attn_with_kvcache(q4, kc4, vc4, cache_seqlens=lens4, num_splits=2, tree_mask=None)
    ops.flash_attn_with_kvcache(q4, kc4, vc4, cache_seqlens=lens4, causal=True, pack_gqa=True, tree_mask=None)
    ops.flash_attn_with_kvcache(q4, kc4, vc4, cache_seqlens=lens4, causal=True, num_splits=1, sliding_window=65, tree_mask=None)
    assert [c[0] for c in stub.calls] == ["tfa_fwd_kvcache_varlen_suggest_splits", "tfa_fwd_kvcache_varlen_workspace", "tfa_fwd_kvcache_varlen",
                                          "tfa_fwd_kvcache_varlen_workspace", "tfa_fwd_kvcache_varlen", "tfa_fwd_kvcache_workspace", "tfa_fwd_kvcache",
                                          "tfa_fwd_kvcache_pack_suggest_splits", "tfa_fwd_kvcache_pack_workspace", "tfa_fwd_kvcache_pack",
                                          "tfa_fwd_kvcache_window_workspace", "tfa_fwd_kvcache_window"]


def test_4d_call_takes_the_tree_entry_point(stub):
    q, kc, vc, lens = _t4()
    words = _meta(2, 4, dtype=torch.int64)
    out, lse = ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, causal=True, return_softmax_lse=True, tree_mask=words)
    assert [c[0] for c in stub.calls] == TREE_CALLS
    pref, vq, mode, tr = stub.calls[0][1]
    assert vq is None and mode == AUTO and (tr._obj.mask, tr._obj.batch_stride, tr._obj.row_stride) == (words.data_ptr(), 4, 1)
    pref, vq, q8, mode, tr, splits = stub.calls[1][1]
    assert vq is None and q8 is None and (mode, splits) == (AUTO, 3)
    pref, vq, q8, mode, tr, splits, meta, ws, stream = stub.calls[2][1]
    p = pref._obj
    assert vq is None and q8 is None and meta is None and ws is not None and (mode, splits) == (AUTO, 3) and tr._obj.mask == words.data_ptr()
    assert (p.B, p.H, p.Hk, p.Nq, p.D, p.capacity, p.is_causal, p.n_new) == (2, 8, 2, 4, 64, 1024, 1, 0)
    assert tuple(out.shape) == (2, 4, 8, 64) and tuple(lse.shape) == (2, 8, 4)
    # any strides: a slice of a wider tensor is handed over as it is
    for pack_gqa, want in ((True, ON), (False, OFF)):
        stub.calls.clear()
        wide = _meta(2, 8, 3, dtype=torch.int64)[:, :4, 1]
        ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, causal=True, num_splits=1, pack_gqa=pack_gqa, tree_mask=wide)
        assert [c[0] for c in stub.calls] == TREE_CALLS[1:]
        tr = stub.calls[-1][1][4]._obj
        assert stub.calls[-1][1][3] == want and stub.calls[-1][1][5] == 1 and stub.calls[-1][1][7] is None and (tr.batch_stride, tr.row_stride) == (24, 3)
    # the bool form is packed on its device into (B, Nq) words
    stub.calls.clear()
    ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, causal=True, num_splits=2, tree_mask=_meta(2, 4, 4, dtype=torch.bool))
    tr = stub.calls[-1][1][4]._obj
    assert stub.calls[-1][0] == "tfa_fwd_kvcache_tree" and (tr.batch_stride, tr.row_stride) == (4, 1)
    # k= / v= ride in the parameter block: the entry point appends first; an fp8 cache brings its struct
    stub.calls.clear()
    kn = _meta(2, 4, 2, 64)
    ops.flash_attn_with_kvcache(q, kc, vc, kn, kn, cache_seqlens=lens, causal=True, num_splits=2, tree_mask=words)
    p = stub.calls[-1][1][0]._obj
    assert stub.calls[-1][0] == "tfa_fwd_kvcache_tree" and p.n_new == 4 and p.k_new is not None
    stub.calls.clear()
    q, kc8, vc8, lens = _t4(cache_dtype=torch.float8_e4m3fn)
    kd = _meta(2, 2, dtype=torch.float32)
    ops.flash_attn_with_kvcache(q, kc8, vc8, cache_seqlens=lens, causal=True, num_splits=1, tree_mask=words, k_descale=kd)
    q8 = stub.calls[-1][1][2]
    assert stub.calls[-1][0] == "tfa_fwd_kvcache_tree" and q8 is not None and q8._obj.format == _lib.TFA_KV_E4M3 and q8._obj.k_descale == kd.data_ptr()


def test_packed_call_takes_the_tree_entry_point(stub):
    q, kc, vc, lens, cu = VA._tensors()
    words = _meta(10, dtype=torch.int64)
    out, lse = ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, causal=True, return_softmax_lse=True, cu_seqlens_q=cu, max_seqlen_q=7, tree_mask=words)
    assert [c[0] for c in stub.calls] == TREE_CALLS
    pref, vref, q8, mode, tr, splits, meta, ws, stream = stub.calls[2][1]
    p, v = pref._obj, vref._obj
    assert q8 is None and meta is None and ws is not None and (mode, splits) == (ON, 3)
    assert (tr._obj.mask, tr._obj.batch_stride, tr._obj.row_stride) == (words.data_ptr(), 0, 1)
    assert (p.B, p.H, p.Hk, p.D, p.capacity, p.is_causal) == (3, 8, 2, 64, 1024, 1)
    assert (v.cu_seqlens_q, v.max_seqlen_q, v.total_q) == (cu.data_ptr(), 7, 10)
    assert tuple(out.shape) == (10, 8, 64) and tuple(lse.shape) == (8, 10)
    # scheduled: the list's size is checked as today, then the one entry point with the list
    stub.calls.clear()
    md = _meta(SA._CountingLib.SIZE, dtype=torch.int32)
    ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, causal=True, num_splits=1, pack_gqa=False, cu_seqlens_q=cu, max_seqlen_q=7, scheduler_metadata=md,
                                tree_mask=_meta(20, dtype=torch.int64)[::2])
    assert [c[0] for c in stub.calls] == ["tfa_kvcache_varlen_schedule_size"] + TREE_CALLS[1:]
    pref, vref, q8, mode, tr, splits, meta, ws, stream = stub.calls[-1][1]
    assert (mode, splits) == (OFF, 1) and meta.value == md.data_ptr() and ws is None and vref._obj.total_q == 10 and tr._obj.row_stride == 2


def test_bool_masks_are_packed_into_words_bit_63_included():
    g = torch.Generator().manual_seed(5)
    m = torch.rand(2, 64, 64, generator=g) < 0.5
    m[0, 63, 63], m[1, 63, 63] = True, False
    w = ops._tree_words("f", m, m.device, 2, 64)
    assert w.dtype == torch.int64 and tuple(w.shape) == (2, 64)
    for b in range(2):
        for t in (0, 1, 31, 32, 62, 63):
            want = sum(1 << s for s in range(64) if m[b, t, s])
            assert int(w[b, t]) & ((1 << 64) - 1) == want
    assert int(w[0, 63]) < 0 <= int(w[1, 63])
    assert torch.equal(ops._tree_words("f", torch.ones(1, 3, 3, dtype=torch.bool).tril(), m.device, 1, 3), torch.tensor([[1, 3, 7]]))
    x = torch.arange(6, dtype=torch.int64).view(2, 3)
    assert ops._tree_words("f", x, x.device, 2, 3) is x and ops._tree_words("f", x.view(6), x.device, None, 6).data_ptr() == x.data_ptr()


def test_wrapper_refusals(stub):
    q, kc, vc, lens, cu = VA._tensors()
    q4, kc4, vc4, lens4 = _t4()
    i64 = torch.int64
    forms = ((q, kc, vc, dict(cache_seqlens=lens, cu_seqlens_q=cu, max_seqlen_q=7), _meta(10, dtype=i64)),
             (q4, kc4, vc4, dict(cache_seqlens=lens4), _meta(2, 4, dtype=i64)))
    for q_, k_, v_, kw, good in forms:
        for bad in (-1, [[1, 3]], "tree", True):
            with pytest.raises(TypeError, match="tree_mask"):
                ops.flash_attn_with_kvcache(q_, k_, v_, causal=True, tree_mask=bad, **kw)
        with pytest.raises(ValueError, match="causal"):
            ops.flash_attn_with_kvcache(q_, k_, v_, causal=False, tree_mask=good, **kw)
        with pytest.raises(ValueError, match="causal"):
            ops.flash_attn_with_kvcache(q_, k_, v_, tree_mask=good, **kw)
        with pytest.raises(ValueError, match="sliding_window"):
            ops.flash_attn_with_kvcache(q_, k_, v_, causal=True, tree_mask=good, sliding_window=65, **kw)
        with pytest.raises(ValueError, match="device"):
            ops.flash_attn_with_kvcache(q_, k_, v_, causal=True, tree_mask=torch.zeros(tuple(good.shape), dtype=i64), **kw)
        for dt in (torch.int32, torch.uint8, torch.float32):
            with pytest.raises(ValueError, match="int64"):
                ops.flash_attn_with_kvcache(q_, k_, v_, causal=True, tree_mask=_meta(*good.shape, dtype=dt), **kw)
    # shapes
    for bad in (_meta(2, 5, dtype=i64), _meta(3, 4, dtype=i64), _meta(8, dtype=i64), _meta(2, 4, 1, dtype=i64), _meta(2, 4, 5, dtype=torch.bool),
                _meta(2, 4, dtype=torch.bool)):
        with pytest.raises(ValueError, match="tree_mask"):
            ops.flash_attn_with_kvcache(q4, kc4, vc4, cache_seqlens=lens4, causal=True, tree_mask=bad)
    for bad in (_meta(9, dtype=i64), _meta(11, dtype=i64), _meta(10, 1, dtype=i64), _meta(3, 7, dtype=i64)):
        with pytest.raises(ValueError, match="tree_mask"):
            ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, causal=True, cu_seqlens_q=cu, max_seqlen_q=7, tree_mask=bad)
    with pytest.raises(ValueError, match="int64 layout"):                                  # a bool mask in the packed form
        ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, causal=True, cu_seqlens_q=cu, max_seqlen_q=7, tree_mask=_meta(10, 10, dtype=torch.bool))
    # more than 64 rows in the 4-D form
    q65, kc65, vc65, lens65 = _t4(Nq=65)
    for bad in (_meta(2, 65, dtype=i64), _meta(2, 65, 65, dtype=torch.bool)):
        with pytest.raises(ValueError, match="64"):
            ops.flash_attn_with_kvcache(q65, kc65, vc65, cache_seqlens=lens65, causal=True, tree_mask=bad)
    with pytest.raises(TypeError):
        ops.flash_attn_with_kvcache(q4, kc4, vc4, None, None, lens4, None, None, True, 0, False, _meta(2, 4, dtype=i64))      # keyword-only
    assert stub.calls == []
