"""CPU tests of the sliding window over a K/V cache (include/tfa.h: tfa_fwd_kvcache_window, _window_plan, _window_workspace, _window_suggest_splits) and of
``flash_attn_with_kvcache(sliding_window=)``: the symbols, plans (the underlying form's grid), refusal codes, the split suggestion, and the wrapper's calls and
refusals against a counting stand-in for the library.  No GPU: plans never launch, refused calls return before any launch."""
import ctypes as C
import inspect

import pytest
import torch

import test_kvcache_sched_abi as SA
import test_kvcache_varlenq_abi as VA
from tiny_flash_attention_amd import _lib, ops

ADDR, CODES, AUTO, ON, OFF = VA.ADDR, VA.CODES, VA.AUTO, VA.ON, VA.OFF
WIN_SYMBOLS = ("tfa_fwd_kvcache_window", "tfa_fwd_kvcache_window_plan", "tfa_fwd_kvcache_window_workspace", "tfa_fwd_kvcache_window_suggest_splits")
_meta = VA._meta


def params4(B=3, H=8, Hk=2, Nq=5, D=64, cap=1024, page=0, causal=True, dtype=_lib.TFA_BF16):
    """A tfa_kvcache_params of the 4-D call: q (B, Nq, H, D), out dense (B, H, Nq, D)."""
    p = _lib.TfaKvcacheParams()
    p.q = p.out = p.lse = p.k_cache = p.v_cache = p.cache_seqlens = ADDR
    p.B, p.H, p.Hk, p.Nq, p.D, p.capacity = B, H, Hk, Nq, D, cap
    p.q_stride[0], p.q_stride[1], p.q_stride[2] = Nq * H * D, D, H * D
    p.o_stride[0], p.o_stride[1], p.o_stride[2] = H * Nq * D, Nq * D, D
    rows = page if page else cap
    for name in ("k_stride", "v_stride"):
        arr = getattr(p, name)
        arr[0], arr[1], arr[2] = rows * Hk * D, D, Hk * D
    if page:
        p.block_table, p.block_table_stride, p.page_size, p.num_pages = ADDR, cap // page, page, B * (cap // page)
    p.softmax_scale, p.is_causal, p.dtype = 0.125, 1 if causal else 0, dtype
    return p


def ref(x):
    return C.byref(x) if x is not None else None


def wplan(p, vq, left, mode=AUTO, splits=1, q8=None, scheduled=0):
    g, b, l = C.c_int(), C.c_int(), C.c_int()
    st = _lib.lib().tfa_fwd_kvcache_window_plan(ref(p), ref(vq), ref(q8), mode, left, splits, scheduled, C.byref(g), C.byref(b), C.byref(l))
    return st, g.value, b.value, l.value


def pack_plan(p, mode=AUTO, splits=1, q8=None):
    g, b, l = C.c_int(), C.c_int(), C.c_int()
    st = _lib.lib().tfa_fwd_kvcache_pack_plan(ref(p), ref(q8), mode, splits, C.byref(g), C.byref(b), C.byref(l))
    return st, g.value, b.value, l.value


def test_symbols_exported_and_version():
    L = _lib.lib()
    for s in WIN_SYMBOLS:
        assert s in _lib.SYMBOLS
        getattr(L, s)
    assert L.tfa_version() == 111
    names = list(inspect.signature(ops.flash_attn_with_kvcache).parameters)
    assert names[-3:] == ["sliding_window", "k_descale", "v_descale"] and names[names.index("sliding_window") - 1] == "scheduler_metadata"
    assert inspect.signature(ops.flash_attn_with_kvcache).parameters["sliding_window"].kind is inspect.Parameter.KEYWORD_ONLY


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("left", [0, 63, 1023, 1 << 30])
def test_window_plan_grid_is_the_underlying_forms(left, splits):
    fp8 = _lib.TfaKvcacheFp8()
    fp8.format = _lib.TFA_KV_E4M3
    for q8 in (None, fp8):
        # 4-D, several rows: tfa_fwd_kvcache_pack_plan's
        for Nq, page in ((5, 0), (130, 128), (33, 0)):
            p = params4(Nq=Nq, page=page)
            for mode in (AUTO, ON, OFF):
                want = pack_plan(p, mode, splits, q8)
                assert want[0] == 0 and wplan(p, None, left, mode, splits, q8) == want
        # 4-D decode: AUTO and ON stream K/V once per K/V head (one workgroup per (b, hk, chunk)), OFF once per query head
        p = params4(Nq=1)
        assert wplan(p, None, left, AUTO, splits, q8) == wplan(p, None, left, ON, splits, q8) == (0, 3 * 2 * splits, 256, 4 * 64 * 64 * 2) == pack_plan(p, AUTO, splits, q8)
        assert wplan(p, None, left, OFF, splits, q8) == (0, 3 * 8 * splits, 256, 4 * 64 * 64 * 2) == pack_plan(p, OFF, splits, q8)
        # packed q, unscheduled and scheduled
        for mq, tq in ((5, 9), (40, 50)):
            p, vq = VA.params(B=3, H=8, Hk=2, D=64, cap=1024, total_q=tq, causal=True), VA.varlen(mq, tq)
            for mode in (AUTO, ON, OFF):
                assert wplan(p, vq, left, mode, splits, q8) == VA.plan(p, vq, mode, splits, q8) and VA.plan(p, vq, mode, splits, q8)[0] == 0
                assert wplan(p, vq, left, mode, splits, q8, scheduled=1) == SA.sched_plan(p, vq, mode, splits, q8)


def test_window_plan_refusals():
    L = _lib.lib()
    p, pv, vq = params4(), VA.params(total_q=64, causal=True), VA.varlen()
    assert wplan(None, None, 3)[0] == wplan(None, vq, 3)[0] == CODES["TFA_ERR_NULL"]
    for left in (-1, -1024):
        assert wplan(p, None, left)[0] == wplan(pv, vq, left)[0] == CODES["TFA_ERR_SHAPE"]
    assert wplan(params4(causal=False), None, 3)[0] == wplan(VA.params(total_q=64, causal=False), vq, 3)[0] == CODES["TFA_ERR_SHAPE"]
    assert wplan(p, None, 3, scheduled=1)[0] == CODES["TFA_ERR_SHAPE"]                      # a list without cu_seqlens_q
    assert L.tfa_fwd_kvcache_window(C.byref(p), None, None, AUTO, 3, 1, ADDR, None, None) == CODES["TFA_ERR_SHAPE"]
    assert L.tfa_fwd_kvcache_window(C.byref(p), None, None, AUTO, -1, 1, None, None, None) == CODES["TFA_ERR_SHAPE"]
    assert L.tfa_fwd_kvcache_window(C.byref(pv), C.byref(vq), None, ON, 3, 1, ADDR + 4, None, None) == CODES["TFA_ERR_ALIGN"]      # the scheduled form's own check
    # every other check is the underlying form's, with its code
    seen = set()
    for bad in (params4(D=12), params4(dtype=_lib.TFA_F32), params4(B=0), params4(H=12, Hk=8), params4(cap=0), params4(Nq=0)):
        for mode in (AUTO, ON, OFF, 7):
            want = pack_plan(bad, mode, 2)[0]
            assert want < 0 and wplan(bad, None, 3, mode, 2)[0] == want
            seen.add(want)
    for bad, v in ((VA.params(D=12, causal=True), vq), (VA.params(causal=True), VA.varlen(0, 64)), (VA.params(causal=True), VA.varlen(16, 0)),
                   (VA.params(total_q=64, dense_out=False, causal=True), vq)):
        want = VA.plan(bad, v, ON, 2)[0]
        assert want < 0 and wplan(bad, v, 3, ON, 2)[0] == want and wplan(bad, v, 3, ON, 2, scheduled=1)[0] == want
        seen.add(want)
    assert len(seen) >= 4
    assert wplan(p, None, 3, AUTO, 0)[0] == CODES["TFA_ERR_SHAPE"]


def test_window_workspace_is_the_underlying_forms():
    L = _lib.lib()
    p = params4(Nq=5)
    pv, vq = VA.params(B=3, H=8, Hk=2, D=64, cap=1024, total_q=9, causal=True), VA.varlen(5, 9)
    for mode in (AUTO, ON, OFF):
        for splits in (1, 2, 5, 64):
            assert L.tfa_fwd_kvcache_window_workspace(C.byref(p), None, None, mode, 99, splits) == L.tfa_fwd_kvcache_pack_workspace(C.byref(p), None, mode, splits)
            assert (L.tfa_fwd_kvcache_window_workspace(C.byref(pv), C.byref(vq), None, mode, 99, splits)
                    == L.tfa_fwd_kvcache_varlen_workspace(C.byref(pv), C.byref(vq), None, mode, splits))
    assert L.tfa_fwd_kvcache_window_workspace(C.byref(p), None, None, AUTO, 99, 2) == 2 * 3 * 8 * 5 * 65
    assert L.tfa_fwd_kvcache_window_workspace(C.byref(p), None, None, AUTO, -1, 2) == CODES["TFA_ERR_SHAPE"]


def test_window_suggest_splits_takes_the_windows_reach_for_the_lengths():
    """The existing rule with min(capacity, round_up(w - 1 + rows, 64) + 64) standing in for the lengths; 256 CUs without a device."""
    L = _lib.lib()

    def at(cap, **kw):
        return params4(B=1, H=32, Hk=8, D=128, cap=cap, **kw)

    # capacity 16384, w = 1024: 1088 keys for one row, 1152 for 2..65 rows — what the plain rule returns at that capacity
    for Nq, reach in ((1, 1088), (2, 1152), (5, 1152), (65, 1152), (130, 1216)):
        for mode in (AUTO, ON, OFF):
            got = L.tfa_fwd_kvcache_window_suggest_splits(C.byref(at(16384, Nq=Nq)), None, mode, 1023)
            assert got == L.tfa_fwd_kvcache_pack_suggest_splits(C.byref(at(reach, Nq=Nq)), mode) == 1
    # a window of 8192 over 16384 keys: the rule at 8256 keys (8 chunks of >= 1024), not at 16384 (16)
    p = at(16384, Nq=1)
    assert L.tfa_fwd_kvcache_window_suggest_splits(C.byref(p), None, AUTO, 8191) == L.tfa_fwd_kvcache_pack_suggest_splits(C.byref(at(8256, Nq=1)), AUTO) == 8
    assert L.tfa_fwd_kvcache_pack_suggest_splits(C.byref(p), AUTO) == 16
    # a window beyond the capacity: the capacity
    assert L.tfa_fwd_kvcache_window_suggest_splits(C.byref(p), None, AUTO, 1 << 30) == 16
    # packed q: tfa_fwd_kvcache_varlen_suggest_splits' rule, rows = max_seqlen_q
    pv, vq = VA.params(B=1, H=32, Hk=8, cap=16384, total_q=1, causal=True), VA.varlen(1, 1)
    small = VA.params(B=1, H=32, Hk=8, cap=8256, total_q=1, causal=True)
    assert (L.tfa_fwd_kvcache_window_suggest_splits(C.byref(pv), C.byref(vq), ON, 8191) == L.tfa_fwd_kvcache_varlen_suggest_splits(C.byref(small), C.byref(vq), ON) == 8)
    assert L.tfa_fwd_kvcache_window_suggest_splits(None, None, AUTO, 3) == 1 and L.tfa_fwd_kvcache_window_suggest_splits(C.byref(p), None, AUTO, -1) == 1


# ---- Python: flash_attn_with_kvcache(sliding_window=) against a counting stand-in for the library ----------------------------------------------------------
class _CountingLib(SA._CountingLib):
    def __getattr__(self, name):
        base = super().__getattr__(name)

        def f(*a):
            r = base(*a)
            if name == "tfa_fwd_kvcache_window_suggest_splits":
                return 3
            if name == "tfa_fwd_kvcache_window_workspace":
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


WINDOW_CALLS = ["tfa_fwd_kvcache_window_suggest_splits", "tfa_fwd_kvcache_window_workspace", "tfa_fwd_kvcache_window"]


def _t4(B=2, Nq=4, H=8, Hk=2, D=64, cap=1024, cache_dtype=torch.bfloat16):
    return _meta(B, Nq, H, D), _meta(B, cap, Hk, D, dtype=cache_dtype), _meta(B, cap, Hk, D, dtype=cache_dtype), _meta(B, dtype=torch.int32)


def test_without_sliding_window_the_calls_are_todays(stub):
    q, kc, vc, lens, cu = VA._tensors()
    ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, causal=True, cu_seqlens_q=cu, max_seqlen_q=7)
    ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, num_splits=3, cu_seqlens_q=cu, max_seqlen_q=7, sliding_window=None)
    q4, kc4, vc4, lens4 = _t4()
    ops.flash_attn_with_kvcache(q4, kc4, vc4, cache_seqlens=lens4, num_splits=2, sliding_window=None)
    ops.flash_attn_with_kvcache(q4, kc4, vc4, cache_seqlens=lens4, causal=True, pack_gqa=True)
    assert [c[0] for c in stub.calls] == ["tfa_fwd_kvcache_varlen_suggest_splits", "tfa_fwd_kvcache_varlen_workspace", "tfa_fwd_kvcache_varlen",
                                          "tfa_fwd_kvcache_varlen_workspace", "tfa_fwd_kvcache_varlen", "tfa_fwd_kvcache_workspace", "tfa_fwd_kvcache",
                                          "tfa_fwd_kvcache_pack_suggest_splits", "tfa_fwd_kvcache_pack_workspace", "tfa_fwd_kvcache_pack"]


def test_4d_call_takes_the_window_entry_point(stub):
    q, kc, vc, lens = _t4()
    out, lse = ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, causal=True, return_softmax_lse=True, sliding_window=65)
    assert [c[0] for c in stub.calls] == WINDOW_CALLS
    pref, vq, mode, left = stub.calls[0][1]
    assert vq is None and mode == AUTO and left == 64
    pref, vq, q8, mode, left, splits = stub.calls[1][1]
    assert vq is None and q8 is None and (mode, left, splits) == (AUTO, 64, 3)
    pref, vq, q8, mode, left, splits, meta, ws, stream = stub.calls[2][1]
    p = pref._obj
    assert vq is None and q8 is None and meta is None and ws is not None and (mode, left, splits) == (AUTO, 64, 3)
    assert (p.B, p.H, p.Hk, p.Nq, p.D, p.capacity, p.is_causal, p.n_new) == (2, 8, 2, 4, 64, 1024, 1, 0)
    assert tuple(out.shape) == (2, 4, 8, 64) and tuple(lse.shape) == (2, 8, 4)
    for pack_gqa, want in ((True, ON), (False, OFF)):
        stub.calls.clear()
        ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, causal=True, num_splits=1, pack_gqa=pack_gqa, sliding_window=1)
        assert [c[0] for c in stub.calls] == WINDOW_CALLS[1:]
        assert stub.calls[-1][1][3:6] == (want, 0, 1) and stub.calls[-1][1][7] is None
    # k= / v= ride in the parameter block: the entry point appends first; an fp8 cache brings its struct
    stub.calls.clear()
    kn = _meta(2, 4, 2, 64)
    ops.flash_attn_with_kvcache(q, kc, vc, kn, kn, cache_seqlens=lens, causal=True, num_splits=2, sliding_window=128)
    p = stub.calls[-1][1][0]._obj
    assert stub.calls[-1][0] == "tfa_fwd_kvcache_window" and p.n_new == 4 and p.k_new is not None and stub.calls[-1][1][4] == 127
    stub.calls.clear()
    q, kc8, vc8, lens = _t4(cache_dtype=torch.float8_e4m3fn)
    kd = _meta(2, 2, dtype=torch.float32)
    ops.flash_attn_with_kvcache(q, kc8, vc8, cache_seqlens=lens, causal=True, num_splits=1, sliding_window=2, k_descale=kd)
    q8 = stub.calls[-1][1][2]
    assert stub.calls[-1][0] == "tfa_fwd_kvcache_window" and q8 is not None and q8._obj.format == _lib.TFA_KV_E4M3 and q8._obj.k_descale == kd.data_ptr()
    assert q8._obj.v_descale is None and stub.calls[-1][1][4] == 1


def test_packed_call_takes_the_window_entry_point(stub):
    q, kc, vc, lens, cu = VA._tensors()
    out, lse = ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, causal=True, return_softmax_lse=True, cu_seqlens_q=cu, max_seqlen_q=7, sliding_window=100)
    assert [c[0] for c in stub.calls] == WINDOW_CALLS
    pref, vref, q8, mode, left, splits, meta, ws, stream = stub.calls[2][1]
    p, v = pref._obj, vref._obj
    assert q8 is None and meta is None and ws is not None and (mode, left, splits) == (ON, 99, 3)
    assert (p.B, p.H, p.Hk, p.D, p.capacity, p.is_causal) == (3, 8, 2, 64, 1024, 1)
    assert (v.cu_seqlens_q, v.max_seqlen_q, v.total_q) == (cu.data_ptr(), 7, 10)
    assert tuple(out.shape) == (10, 8, 64) and tuple(lse.shape) == (8, 10)
    # scheduled: the list's size is checked as today, then the one entry point with the list
    stub.calls.clear()
    md = _meta(SA._CountingLib.SIZE, dtype=torch.int32)
    ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, causal=True, num_splits=1, pack_gqa=False, cu_seqlens_q=cu, max_seqlen_q=7, scheduler_metadata=md,
                                sliding_window=1)
    assert [c[0] for c in stub.calls] == ["tfa_kvcache_varlen_schedule_size"] + WINDOW_CALLS[1:]
    pref, vref, q8, mode, left, splits, meta, ws, stream = stub.calls[-1][1]
    assert (mode, left, splits) == (OFF, 0, 1) and meta.value == md.data_ptr() and ws is None and vref._obj.total_q == 10


def test_a_window_that_reaches_every_key_takes_the_plain_entry_points(stub):
    q, kc, vc, lens, cu = VA._tensors()
    q4, kc4, vc4, lens4 = _t4()
    for w in (1025, 1 << 40):                                # capacity 1024: w - 1 >= capacity
        ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, causal=True, num_splits=3, cu_seqlens_q=cu, max_seqlen_q=7, sliding_window=w)
        ops.flash_attn_with_kvcache(q4, kc4, vc4, cache_seqlens=lens4, causal=True, num_splits=2, sliding_window=w)
    assert [c[0] for c in stub.calls] == ["tfa_fwd_kvcache_varlen_workspace", "tfa_fwd_kvcache_varlen", "tfa_fwd_kvcache_workspace", "tfa_fwd_kvcache"] * 2
    stub.calls.clear()
    ops.flash_attn_with_kvcache(q4, kc4, vc4, cache_seqlens=lens4, causal=True, num_splits=2, sliding_window=1024)      # w - 1 = 1023 < capacity: the window
    assert stub.calls[-1][0] == "tfa_fwd_kvcache_window" and stub.calls[-1][1][4] == 1023


def test_wrapper_refusals(stub):
    q, kc, vc, lens, cu = VA._tensors()
    q4, kc4, vc4, lens4 = _t4()
    forms = ((q, kc, vc, dict(cache_seqlens=lens, cu_seqlens_q=cu, max_seqlen_q=7)), (q4, kc4, vc4, dict(cache_seqlens=lens4)))
    for q_, k_, v_, kw in forms:
        for bad in (torch.tensor(64), 64.0, "64", True, (63, 0)):
            with pytest.raises(TypeError, match="sliding_window"):
                ops.flash_attn_with_kvcache(q_, k_, v_, causal=True, sliding_window=bad, **kw)
        for bad in (0, -1):
            with pytest.raises(ValueError, match="sliding_window"):
                ops.flash_attn_with_kvcache(q_, k_, v_, causal=True, sliding_window=bad, **kw)
        with pytest.raises(ValueError, match="causal"):
            ops.flash_attn_with_kvcache(q_, k_, v_, causal=False, sliding_window=64, **kw)
        with pytest.raises(ValueError, match="causal"):
            ops.flash_attn_with_kvcache(q_, k_, v_, sliding_window=1 << 40, **kw)            # also where the plain entry points would run
        # window_size stays refused, and names the keyword that is not
        for ws in ((64, 0), (-1, 0), (0, -1)):
            with pytest.raises(NotImplementedError, match="window_size") as e:
                ops.flash_attn_with_kvcache(q_, k_, v_, causal=True, window_size=ws, **kw)
            assert "sliding_window" in str(e.value)
        with pytest.raises(NotImplementedError, match="window_size"):
            ops.flash_attn_with_kvcache(q_, k_, v_, causal=True, window_size=(64, 0), sliding_window=65, **kw)
    with pytest.raises(TypeError):
        ops.flash_attn_with_kvcache(q4, kc4, vc4, None, None, lens4, None, None, True, 0, False, 64)      # keyword-only
    assert stub.calls == []
