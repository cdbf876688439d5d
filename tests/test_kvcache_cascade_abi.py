"""CPU tests of shared-prefix (cascade) attention (include/tfa.h: tfa_fwd_kvcache_cascade, _workspace, _plan, _suggest_splits; struct tfa_kvcache_cascade) and of
``flash_attn_with_kvcache_cascade``: the symbols, the struct's layout against the header, the workspace formula, each level's plan against the packed-q call it stands
for, every refusal code, and the wrapper's calls and refusals against a counting stand-in for the library.  No GPU: plans never launch, refused calls return before
any launch."""
import ctypes as C
import inspect
import os
import subprocess
import tempfile

import pytest
import torch

import test_kvcache_sched_abi as SA
import test_kvcache_varlenq_abi as VA
import tiny_flash_attention_amd as tfa
from tiny_flash_attention_amd import _lib, ops

ROOT, ADDR, CODES, AUTO, ON, OFF = VA.ROOT, VA.ADDR, VA.CODES, VA.AUTO, VA.ON, VA.OFF
CS_SYMBOLS = ("tfa_fwd_kvcache_cascade", "tfa_fwd_kvcache_cascade_workspace", "tfa_fwd_kvcache_cascade_plan", "tfa_fwd_kvcache_cascade_suggest_splits")
_meta = VA._meta


def ref(x):
    return C.byref(x) if x is not None else None


def cascade(groups=2, pmb=4, pmq=12, cu=ADDR, lens=ADDR, table=ADDR, stride=None, reserved=0):
    cs = _lib.TfaKvcacheCascade()
    cs.prefix_cu_seqlens_q, cs.prefix_seqlens, cs.prefix_block_table = cu, lens, table
    cs.prefix_block_table_stride = pmb if stride is None else stride
    cs.num_groups, cs.prefix_max_blocks, cs.prefix_max_seqlen_q, cs.reserved_ = groups, pmb, pmq, reserved
    return cs


def params(**kw):
    kw.setdefault("page", 64)
    kw.setdefault("causal", True)
    return VA.params(**kw)


def cplan(p, vq, cs, level, mode=ON, splits=1, psplits=1, sched=0, psched=0):
    g, b, l = C.c_int(), C.c_int(), C.c_int()
    st = _lib.lib().tfa_fwd_kvcache_cascade_plan(ref(p), ref(vq), ref(cs), mode, splits, psplits, sched, psched, level, C.byref(g), C.byref(b), C.byref(l))
    return st, g.value, b.value, l.value


def cws(p, vq, cs, mode=ON, splits=1, psplits=1):
    return _lib.lib().tfa_fwd_kvcache_cascade_workspace(ref(p), ref(vq), ref(cs), mode, splits, psplits)


def level0(p, vq, cs):
    """Level 0 as the packed-q call it stands for: the groups as sequences, non-causal, prefix_max_blocks pages of capacity."""
    p0 = params(B=cs.num_groups, H=p.H, Hk=p.Hk, D=p.D, cap=cs.prefix_max_blocks * p.page_size, total_q=vq.total_q, page=p.page_size, num_pages=p.num_pages,
                causal=False, dtype=p.dtype)
    return p0, VA.varlen(cs.prefix_max_seqlen_q, vq.total_q)


def test_symbols_exported_version_and_export():
    L = _lib.lib()
    for s in CS_SYMBOLS:
        assert s in _lib.SYMBOLS
        getattr(L, s)
    assert L.tfa_version() == 111
    assert tfa.flash_attn_with_kvcache_cascade is ops.flash_attn_with_kvcache_cascade and "flash_attn_with_kvcache_cascade" in tfa.__all__
    sig = inspect.signature(ops.flash_attn_with_kvcache_cascade).parameters
    assert list(sig)[:3] == ["q", "k_cache", "v_cache"] and all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in list(sig.items())[3:])
    assert list(sig)[3:] == ["cu_seqlens_q", "max_seqlen_q", "cache_seqlens", "block_table", "prefix_cu_seqlens_q", "prefix_max_seqlen_q", "prefix_seqlens",
                             "prefix_block_table", "softmax_scale", "causal", "num_splits", "prefix_num_splits", "return_softmax_lse", "pack_gqa",
                             "scheduler_metadata", "prefix_scheduler_metadata"]
    assert sig["causal"].default is True and sig["num_splits"].default == 0 and sig["prefix_num_splits"].default == 0
    # flash_attn_with_kvcache itself took no keyword
    assert "prefix_seqlens" not in inspect.signature(ops.flash_attn_with_kvcache).parameters


def test_struct_layout_against_the_header_and_symbols_link():
    fields = ["prefix_cu_seqlens_q", "prefix_seqlens", "prefix_block_table", "prefix_block_table_stride", "num_groups", "prefix_max_blocks", "prefix_max_seqlen_q",
              "reserved_"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include <string.h>\n#include "tfa.h"\n'
           "int main(void) {\n"
           "  tfa_kvcache_params p; tfa_kvcache_varlen_q v; tfa_kvcache_cascade c; int a = 0, b = 0;\n"
           "  memset(&p, 0, sizeof p); memset(&v, 0, sizeof v); memset(&c, 0, sizeof c);\n"
           "  if (tfa_fwd_kvcache_cascade(&p, &v, 0, TFA_PACK_GQA_AUTO, 1, 1, 0, 0, 0, 0) != TFA_ERR_NULL) return 2;\n"
           "  if (tfa_fwd_kvcache_cascade_plan(&p, &v, &c, TFA_PACK_GQA_ON, 1, 1, 0, 0, 0, &a, 0, 0) != TFA_ERR_NULL) return 3;\n"
           "  if (tfa_fwd_kvcache_cascade_workspace(0, &v, &c, TFA_PACK_GQA_AUTO, 1, 1) != TFA_ERR_NULL) return 4;\n"
           "  if (tfa_fwd_kvcache_cascade_suggest_splits(&p, &v, &c, TFA_PACK_GQA_AUTO, &a, &b) != TFA_ERR_NULL) return 5;\n"
           "  if (tfa_version() != 111) return 6;\n"
           '  printf("%zu ' + "%zu " * len(fields) + '%zu %zu", sizeof(tfa_kvcache_cascade), '
           + ", ".join(f"offsetof(tfa_kvcache_cascade, {f})" for f in fields) + ", sizeof(tfa_kvcache_params), sizeof(tfa_kvcache_varlen_q));\n"
           "  return 0;\n}\n")
    libdir = os.path.dirname(_lib.LIB_PATH)
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.check_call(["cc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe,
                               f"-L{libdir}", "-ltfa_hip", f"-Wl,-rpath,{libdir}"])
        got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    S = _lib.TfaKvcacheCascade
    assert [f[0] for f in S._fields_] == fields
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in fields] + [C.sizeof(_lib.TfaKvcacheParams), C.sizeof(_lib.TfaKvcacheVarlenQ)]
    assert got[:9] == [48, 0, 8, 16, 24, 32, 36, 40, 44]
    assert C.sizeof(_lib.TfaKvcacheParams) == 9 * 8 + 10 * 4 + 19 * 8 + 4 * 4 and C.sizeof(_lib.TfaKvcacheVarlenQ) == 24      # no existing struct moved


@pytest.mark.parametrize("splits,psplits", [(1, 1), (1, 3), (2, 1), (2, 3), (64, 64)])
def test_workspace_formula(splits, psplits):
    """(ns0 + ns1) * H * total_q * (D + 1) floats, ns the chunk count after each level's own clamp min(splits, capacity / 64) — never 0: the call always merges."""
    p, vq, cs = params(B=5, H=8, Hk=2, D=64, cap=512, total_q=40), VA.varlen(16, 40), cascade(groups=2, pmb=4, pmq=30)
    ns1, ns0 = min(splits, 512 // 64), min(psplits, 4 * 64 // 64)
    for mode in (AUTO, ON, OFF):
        assert cws(p, vq, cs, mode, splits, psplits) == (ns0 + ns1) * 8 * 40 * 65
    assert cws(p, vq, cs, ON, 1, 1) == 2 * 8 * 40 * 65 and L_varlen_ws(p, vq, 1) == 0


def L_varlen_ws(p, vq, s):
    return _lib.lib().tfa_fwd_kvcache_varlen_workspace(C.byref(p), C.byref(vq), None, ON, s)


@pytest.mark.parametrize("splits,psplits", [(1, 1), (2, 3), (3, 1)])
@pytest.mark.parametrize("causal", [True, False])
def test_plan_per_level_is_the_packed_q_calls(splits, psplits, causal):
    for (H, Hk, D), (mq, pmq, tq) in (((8, 2, 64), (5, 12, 20)), ((4, 4, 128), (40, 150, 160)), ((16, 4, 128), (33, 71, 200))):
        p, vq, cs = params(B=6, H=H, Hk=Hk, D=D, cap=1024, total_q=tq, causal=causal), VA.varlen(mq, tq), cascade(groups=3, pmb=5, pmq=pmq)
        p0, vq0 = level0(p, vq, cs)
        for mode in (AUTO, ON, OFF):
            want1, want0 = VA.plan(p, vq, mode, splits), VA.plan(p0, vq0, mode, psplits)
            assert want1[0] == 0 and want0[0] == 0
            assert cplan(p, vq, cs, 1, mode, splits, psplits) == want1
            assert cplan(p, vq, cs, 0, mode, splits, psplits) == want0
            assert cplan(p, vq, cs, 1, mode, splits, psplits, sched=1) == SA.sched_plan(p, vq, mode, splits)
            assert cplan(p, vq, cs, 0, mode, splits, psplits, psched=1) == SA.sched_plan(p0, vq0, mode, psplits)
            assert cplan(p, vq, cs, 1, mode, splits, psplits, psched=1) == want1       # the other level's list changes nothing


def test_split_suggestion_is_each_levels_own():
    L = _lib.lib()
    p, vq, cs = params(B=64, H=32, Hk=8, D=128, cap=256, total_q=64, page=256), VA.varlen(1, 64), cascade(groups=4, pmb=32, pmq=16)
    p0, vq0 = level0(p, vq, cs)
    s1, s0 = C.c_int(-1), C.c_int(-1)
    assert L.tfa_fwd_kvcache_cascade_suggest_splits(C.byref(p), C.byref(vq), C.byref(cs), ON, C.byref(s1), C.byref(s0)) == 0
    assert s1.value == L.tfa_fwd_kvcache_varlen_suggest_splits(C.byref(p), C.byref(vq), ON) >= 1
    assert s0.value == L.tfa_fwd_kvcache_varlen_suggest_splits(C.byref(p0), C.byref(vq0), ON) > 1      # 4 groups x 8 K/V heads over 8192 keys: the level is split
    assert L.tfa_fwd_kvcache_cascade_suggest_splits(C.byref(p), C.byref(vq), C.byref(cs), ON, None, C.byref(s0)) == CODES["TFA_ERR_NULL"]
    assert L.tfa_fwd_kvcache_cascade_suggest_splits(C.byref(p), C.byref(vq), None, ON, C.byref(s1), C.byref(s0)) == CODES["TFA_ERR_NULL"]


def test_refusal_codes():
    L = _lib.lib()
    p, vq, cs = params(total_q=64), VA.varlen(), cascade()
    every = lambda p_, vq_, cs_, **kw: {cplan(p_, vq_, cs_, 0, **kw)[0], cplan(p_, vq_, cs_, 1, **kw)[0], cws(p_, vq_, cs_, **{k: v for k, v in kw.items() if k in ("mode", "splits", "psplits")})}      # noqa: E731
    assert every(p, vq, cs) - {cws(p, vq, cs)} == {0} and cws(p, vq, cs) > 0
    # NULL: cs, each member, either struct, a contiguous cache
    for bad in (None, cascade(cu=None), cascade(lens=None), cascade(table=None)):
        assert every(p, vq, bad) == {CODES["TFA_ERR_NULL"]}
    assert every(None, vq, cs) == every(p, None, cs) == {CODES["TFA_ERR_NULL"]}
    assert every(VA.params(total_q=64, causal=True), vq, cs) == {CODES["TFA_ERR_NULL"]}
    # SHAPE: counts, reserved_, splits, the level
    for bad in (cascade(groups=0), cascade(groups=-1), cascade(pmb=0), cascade(pmq=0), cascade(pmq=-3), cascade(reserved=1)):
        assert every(p, vq, bad) == {CODES["TFA_ERR_SHAPE"]}
    assert every(p, vq, cs, splits=0) == every(p, vq, cs, psplits=0) == every(p, vq, cs, mode=7) == {CODES["TFA_ERR_SHAPE"]}
    assert cplan(p, vq, cs, 2)[0] == cplan(p, vq, cs, -1)[0] == CODES["TFA_ERR_SHAPE"]
    # ALIGN: each index array
    for bad in (cascade(cu=ADDR + 2), cascade(lens=ADDR + 1), cascade(table=ADDR + 2)):
        assert every(p, vq, bad) == {CODES["TFA_ERR_ALIGN"]}
    # STRIDE: a table row shorter than its blocks; an out the merge cannot write — at ONE chunk per level too
    assert every(p, vq, cascade(pmb=4, stride=3)) == {CODES["TFA_ERR_STRIDE"]}
    loose = params(total_q=64, dense_out=False)
    assert every(loose, vq, cs) == {CODES["TFA_ERR_STRIDE"]} and VA.plan(loose, vq, ON, 1)[0] == 0
    # the packed-q call's own refusals keep their codes
    seen = set()
    for bad, v in ((params(D=12), vq), (params(dtype=_lib.TFA_F32), vq), (params(B=0), vq), (params(H=12, Hk=8), vq), (params(), VA.varlen(0, 64)),
                   (params(), VA.varlen(16, 0)), (params(page=96), vq)):
        want = VA.plan(bad, v, ON, 2)[0]
        assert want < 0 and every(bad, v, cs, splits=2) == {want}
        seen.add(want)
    assert len(seen) >= 3
    knew = params(total_q=64)
    knew.k_new = knew.v_new = ADDR
    knew.n_new = 1
    assert every(knew, vq, cs) == {VA.plan(knew, vq, ON, 1)[0]} and VA.plan(knew, vq, ON, 1)[0] < 0
    # the call itself: refused before anything is launched (no GPU here)
    call = lambda p_, vq_, cs_, s=1, ps=1, md=None, pmd=None, ws=ADDR: L.tfa_fwd_kvcache_cascade(ref(p_), ref(vq_), ref(cs_), ON, s, ps, md, pmd, ws, None)      # noqa: E731
    assert call(p, vq, None) == call(p, vq, cs, ws=None) == CODES["TFA_ERR_NULL"]
    assert call(p, vq, cascade(reserved=1)) == call(p, vq, cs, s=0) == CODES["TFA_ERR_SHAPE"]
    assert call(p, vq, cs, ws=ADDR + 4) == call(p, vq, cs, md=ADDR + 4) == call(p, vq, cs, pmd=ADDR + 4) == CODES["TFA_ERR_ALIGN"]
    assert call(loose, vq, cs) == CODES["TFA_ERR_STRIDE"]


# ---- Python: flash_attn_with_kvcache_cascade against a counting stand-in for the library -----------------------------------------------------------------------
class _CountingLib(SA._CountingLib):
    def __getattr__(self, name):
        base = super().__getattr__(name)

        def f(*a):
            r = base(*a)
            if name == "tfa_fwd_kvcache_cascade_suggest_splits":
                a[4]._obj.value, a[5]._obj.value = 2, 7
                return 0
            if name == "tfa_fwd_kvcache_cascade_workspace":
                p, vq, s, ps = a[0]._obj, a[1]._obj, a[4], a[5]
                return (s + ps) * p.H * vq.total_q * (p.D + 1)
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


def _tensors(B=5, Gn=2, total_q=10, H=8, Hk=2, D=64, page=128, pages=40, mb=4, pmb=6, dtype=torch.bfloat16):
    i32 = torch.int32
    return dict(q=_meta(total_q, H, D, dtype=dtype), k=_meta(pages, page, Hk, D, dtype=dtype), v=_meta(pages, page, Hk, D, dtype=dtype),
                kw=dict(cu_seqlens_q=_meta(B + 1, dtype=i32), max_seqlen_q=3, cache_seqlens=_meta(B, dtype=i32), block_table=_meta(B, mb, dtype=i32),
                        prefix_cu_seqlens_q=_meta(Gn + 1, dtype=i32), prefix_max_seqlen_q=7, prefix_seqlens=_meta(Gn, dtype=i32),
                        prefix_block_table=_meta(Gn, pmb, dtype=i32)))


CALLS = ["tfa_fwd_kvcache_cascade_suggest_splits", "tfa_fwd_kvcache_cascade_workspace", "tfa_fwd_kvcache_cascade"]


def test_wrapper_makes_exactly_the_expected_calls(stub):
    t = _tensors()
    q, k, v, kw = t["q"], t["k"], t["v"], t["kw"]
    out, lse = ops.flash_attn_with_kvcache_cascade(q, k, v, return_softmax_lse=True, **kw)
    assert [c[0] for c in stub.calls] == CALLS
    pref, vref, cref, mode = stub.calls[0][1][:4]
    assert mode == ON
    pref, vref, cref, mode, splits, psplits = stub.calls[1][1]
    assert (mode, splits, psplits) == (ON, 2, 7)                                  # the library's suggestion, level 1 then level 0
    pref, vref, cref, mode, splits, psplits, md, pmd, ws, stream = stub.calls[2][1]
    p, vq, cs = pref._obj, vref._obj, cref._obj
    assert (mode, splits, psplits) == (ON, 2, 7) and md is None and pmd is None and ws is not None
    assert (p.B, p.H, p.Hk, p.D, p.capacity, p.is_causal, p.n_new, p.page_size, p.num_pages) == (5, 8, 2, 64, 4 * 128, 1, 0, 128, 40)
    assert p.k_new is None and p.v_new is None and p.block_table == kw["block_table"].data_ptr() and p.block_table_stride == 4
    assert p.cache_seqlens == kw["cache_seqlens"].data_ptr() and p.k_cache == k.data_ptr() and p.v_cache == v.data_ptr() and p.q == q.data_ptr()
    assert list(p.q_stride)[1:] == [64, 8 * 64] and list(p.o_stride)[1:] == [10 * 64, 64] and list(p.k_stride) == [128 * 2 * 64, 64, 2 * 64]
    assert (vq.cu_seqlens_q, vq.max_seqlen_q, vq.total_q) == (kw["cu_seqlens_q"].data_ptr(), 3, 10)
    assert (cs.prefix_cu_seqlens_q, cs.prefix_seqlens, cs.prefix_block_table) == tuple(kw[n].data_ptr() for n in ("prefix_cu_seqlens_q", "prefix_seqlens", "prefix_block_table"))
    assert (cs.prefix_block_table_stride, cs.num_groups, cs.prefix_max_blocks, cs.prefix_max_seqlen_q, cs.reserved_) == (6, 2, 6, 7, 0)
    assert tuple(out.shape) == (10, 8, 64) and tuple(lse.shape) == (8, 10) and out.stride() == (64, 10 * 64, 1) and lse.dtype == torch.float32
    # given split counts ask nothing; one given count keeps the other level's suggestion; causal / pack_gqa / strided tables go through
    stub.calls.clear()
    wide = _meta(2, 9, dtype=torch.int32)[:, :6]
    res = ops.flash_attn_with_kvcache_cascade(q, k, v, **dict(kw, prefix_block_table=wide), num_splits=3, prefix_num_splits=1, causal=False, pack_gqa=False)
    assert [c[0] for c in stub.calls] == CALLS[1:] and stub.calls[-1][1][3:6] == (OFF, 3, 1) and isinstance(res, torch.Tensor)
    assert stub.calls[-1][1][0]._obj.is_causal == 0 and stub.calls[-1][1][2]._obj.prefix_block_table_stride == 9
    stub.calls.clear()
    ops.flash_attn_with_kvcache_cascade(q, k, v, **kw, prefix_num_splits=4, pack_gqa=True)
    assert [c[0] for c in stub.calls] == CALLS and stub.calls[-1][1][3:6] == (ON, 2, 4)
    # the lists: each level's size is checked, then both pointers ride in the one call
    stub.calls.clear()
    md, pmd = _meta(SA._CountingLib.SIZE, dtype=torch.int32), _meta(SA._CountingLib.SIZE, dtype=torch.int32)
    ops.flash_attn_with_kvcache_cascade(q, k, v, **kw, num_splits=1, prefix_num_splits=1, scheduler_metadata=md, prefix_scheduler_metadata=pmd)
    assert [c[0] for c in stub.calls] == ["tfa_kvcache_varlen_schedule_size"] * 2 + CALLS[1:]
    (p1, v1, _, cz1), (p0, v0, _, cz0) = stub.calls[0][1], stub.calls[1][1]
    assert (p1._obj.B, v1._obj.max_seqlen_q, cz1) == (5, 3, 1) and (p0._obj.B, v0._obj.max_seqlen_q, cz0) == (2, 7, 0)
    assert stub.calls[-1][1][6].value == md.data_ptr() and stub.calls[-1][1][7].value == pmd.data_ptr()


def test_wrapper_refusals_come_before_any_library_call(stub):
    t = _tensors()
    q, k, v, kw = t["q"], t["k"], t["v"], t["kw"]
    call = lambda q_=q, k_=k, v_=v, **over: ops.flash_attn_with_kvcache_cascade(q_, k_, v_, **dict(kw, **over))      # noqa: E731
    i32 = torch.int32
    with pytest.raises(ValueError, match="packed"):
        call(_meta(5, 2, 8, 64))
    with pytest.raises(ValueError, match="contiguous cache"):
        call(block_table=None)
    with pytest.raises(ValueError, match="contiguous cache"):
        call(prefix_block_table=None)
    # B or Gn differ between a level's three arrays
    for bad in (dict(cache_seqlens=_meta(4, dtype=i32)), dict(block_table=_meta(6, 4, dtype=i32)), dict(cu_seqlens_q=_meta(5, dtype=i32))):
        with pytest.raises(ValueError, match="cache_seqlens|block_table"):
            call(**bad)
    for bad in (dict(prefix_seqlens=_meta(3, dtype=i32)), dict(prefix_block_table=_meta(3, 6, dtype=i32)), dict(prefix_cu_seqlens_q=_meta(4, dtype=i32))):
        with pytest.raises(ValueError, match="prefix_seqlens|prefix_block_table"):
            call(**bad)
    # dtype, device, contiguity of every index array
    shapes = dict(cu_seqlens_q=(6,), cache_seqlens=(5,), block_table=(5, 4), prefix_cu_seqlens_q=(3,), prefix_seqlens=(2,), prefix_block_table=(2, 6))
    for name, shape in shapes.items():
        with pytest.raises(ValueError, match=name):
            call(**{name: _meta(*shape, dtype=torch.int64)})
        with pytest.raises(ValueError, match=name):
            call(**{name: torch.zeros(shape, dtype=i32)})                          # another device
        with pytest.raises(ValueError, match=name):
            call(**{name: [0] * shape[0]})
        strided = _meta(*(shape[:-1] + (2 * shape[-1],)), dtype=i32)[..., ::2]
        with pytest.raises(ValueError, match=name):
            call(**{name: strided})
    for name in ("max_seqlen_q", "prefix_max_seqlen_q"):
        for bad in (None, 0, -2, 3.0, True, "7"):
            with pytest.raises(ValueError, match=name):
                call(**{name: bad})
    with pytest.raises(ValueError, match="num_splits"):
        call(num_splits=-1)
    with pytest.raises(ValueError, match="prefix_num_splits"):
        call(prefix_num_splits=-1)
    k8 = _meta(40, 128, 2, 64, dtype=torch.float8_e4m3fn)
    with pytest.raises(TypeError, match="fp8"):
        call(k_=k8, v_=k8)
    with pytest.raises(TypeError, match="share one dtype"):
        call(k_=_meta(40, 128, 2, 64, dtype=torch.float16), v_=_meta(40, 128, 2, 64, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="not differentiable"):
        call(q_=torch.empty(10, 8, 64, dtype=torch.bfloat16, device="meta", requires_grad=True))
    with pytest.raises(ValueError, match="head dims up to 128"):
        call(q_=_meta(10, 8, 256), k_=_meta(40, 128, 2, 256), v_=_meta(40, 128, 2, 256))
    with pytest.raises(ValueError, match="no fp32"):
        call(q_=_meta(10, 8, 64, dtype=torch.float32), k_=_meta(40, 128, 2, 64, dtype=torch.float32), v_=_meta(40, 128, 2, 64, dtype=torch.float32))
    with pytest.raises(ValueError, match="page size"):
        call(k_=_meta(40, 96, 2, 64), v_=_meta(40, 96, 2, 64))
    with pytest.raises(TypeError, match="pack_gqa"):
        call(pack_gqa="yes")
    with pytest.raises(TypeError, match="prefix_scheduler_metadata"):
        call(prefix_scheduler_metadata=[1, 2])
    with pytest.raises(ValueError, match="scheduler_metadata"):
        call(scheduler_metadata=_meta(SA._CountingLib.SIZE, dtype=torch.int64))
    with pytest.raises(TypeError):
        ops.flash_attn_with_kvcache_cascade(q, k, v, kw["cu_seqlens_q"])             # keyword-only
    assert stub.calls == []
    with pytest.raises(ValueError, match="built for another batch"):                # (the size of a list is the library's host-side answer)
        call(scheduler_metadata=_meta(SA._CountingLib.SIZE + 2, dtype=i32))
    assert [c[0] for c in stub.calls] == ["tfa_kvcache_varlen_schedule_size"]
