"""CPU tests of paged K/V in the packed variable-length forward (include/tfa.h: tfa_fwd_varlen_paged, _plan, _variant, _rounding_rule, struct tfa_paged_kv) and of
the ``block_table`` keyword of ``flash_attn_varlen_func`` / ``ops.flash_attn_varlen_fwd``: symbols, struct layouts against a compiled C snippet, plans and
variants against tfa_fwd_varlen's, every refusal code, and the Python wrapper against a counting stand-in for the library.  No GPU: plans never launch,
refused calls return before any launch, lengths and table are never read on the host (a stand-in address serves)."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest
import torch

from tiny_flash_attention_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDR = 0x10000          # a 16-byte aligned stand-in for device pointers (plans never dereference them)
CODES = {"TFA_ERR_NULL": -1, "TFA_ERR_DTYPE": -2, "TFA_ERR_HEAD_DIM": -3, "TFA_ERR_SHAPE": -4, "TFA_ERR_STRIDE": -5, "TFA_ERR_ALIGN": -6,
         "TFA_ERR_VARIANT": -7, "TFA_ERR_SCALE": -8}
SYMBOLS = ("tfa_fwd_varlen_paged", "tfa_fwd_varlen_paged_plan", "tfa_fwd_varlen_paged_variant", "tfa_fwd_varlen_paged_rounding_rule")


def params(B=8, H=32, Hk=8, D=128, max_q=512, max_k=8192, total_q=4096, page=256, num_pages=300, max_blocks=32, causal=True, dtype=_lib.TFA_BF16,
           head_major=False):
    """tfa_varlen_fwd_params over a (num_pages, page, Hk, D) pool — or its (num_pages, Hk, page, D) memory as a permuted view — and its tfa_paged_kv"""
    p = _lib.TfaVarlenFwdParams()
    p.q = p.k = p.v = p.out = p.lse = p.cu_seqlens_q = p.cu_seqlens_k = ADDR
    p.B, p.H, p.Hk, p.D = B, H, Hk, D
    p.max_seqlen_q, p.max_seqlen_k, p.total_q, p.total_k = max_q, max_k, total_q, 0
    p.q_stride[0], p.q_stride[1] = D, H * D
    p.o_stride[0], p.o_stride[1] = D, H * D
    for name in ("k_stride", "v_stride"):
        getattr(p, name)[0], getattr(p, name)[1] = (page * D, D) if head_major else (D, Hk * D)
    p.softmax_scale, p.is_causal = 0.125, int(causal)
    p.dtype = p.out_dtype = dtype
    pg = _lib.TfaPagedKv()
    pg.block_table, pg.table_stride, pg.max_blocks = ADDR, max_blocks, max_blocks
    pg.page_size, pg.num_pages = page, num_pages
    pg.k_page_stride = pg.v_page_stride = page * Hk * D
    return p, pg


def plan(p, pg):
    g, b, l = C.c_int(), C.c_int(), C.c_int()
    st = _lib.lib().tfa_fwd_varlen_paged_plan(C.byref(p), C.byref(pg) if pg is not None else None, C.byref(g), C.byref(b), C.byref(l))
    return st, g.value, b.value, l.value


def plan_contiguous(p):
    """tfa_fwd_varlen_plan of the same sizes: the keys contiguous (total_k rows of Hk heads)"""
    c = _lib.TfaVarlenFwdParams.from_buffer_copy(p)
    c.total_k = c.B * c.max_seqlen_k
    for name in ("k_stride", "v_stride"):
        getattr(c, name)[0], getattr(c, name)[1] = c.D, c.Hk * c.D
    g, b, l = C.c_int(), C.c_int(), C.c_int()
    st = _lib.lib().tfa_fwd_varlen_plan(C.byref(c), C.byref(g), C.byref(b), C.byref(l))
    return (st, g.value, b.value, l.value), _lib.lib().tfa_fwd_varlen_variant(C.byref(c))


def test_symbols_exported_and_version():
    L = _lib.lib()
    for s in SYMBOLS:
        assert s in _lib.SYMBOLS
        getattr(L, s)
    assert L.tfa_version() == 111


def test_struct_layouts_match_the_header():
    """sizeof(tfa_varlen_fwd_params) is what it was (176 bytes: the struct did not grow for the page arguments) and tfa_paged_kv's size and offsets equal the
    ctypes mirror's (a C program prints them)."""
    fields = [f for f, _ in _lib.TfaPagedKv._fields_]
    prints = "".join(f' printf(" %zu", offsetof(tfa_paged_kv, {f}));' for f in fields)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "tfa.h"\nint main(void) { printf("%zu %zu", sizeof(tfa_varlen_fwd_params), sizeof(tfa_paged_kv));'
           + prints + " return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert got[0] == C.sizeof(_lib.TfaVarlenFwdParams) == 176
    assert got[1] == C.sizeof(_lib.TfaPagedKv) == 48
    assert got[2:] == [getattr(_lib.TfaPagedKv, f).offset for f in fields]


@pytest.mark.parametrize("B,H,Hk,D,max_q,max_k", [(8, 32, 8, 128, 512, 8192), (4, 32, 8, 128, 4096, 4096), (7, 8, 2, 64, 200, 1000), (16, 16, 16, 96, 2048, 2048),
                                                   (2, 4, 1, 40, 1, 300)])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("page", [64, 256])
def test_plan_and_variant_are_the_contiguous_calls(B, H, Hk, D, max_q, max_k, causal, page):
    """_plan reports tfa_fwd_varlen_plan's grid / block / LDS for the same sizes, _variant is tfa_fwd_varlen_variant's (30 or 32), both pool layouts; the rule is
    TFA_RULE_LAZY for both types (per-tile descriptors: the compiler-scheduled tile bodies)."""
    L = _lib.lib()
    for dtype in (_lib.TFA_BF16, _lib.TFA_F16):
        for head_major in (False, True):
            p, pg = params(B=B, H=H, Hk=Hk, D=D, max_q=max_q, max_k=max_k, total_q=B * max_q, page=page, max_blocks=(max_k + page - 1) // page, causal=causal,
                           dtype=dtype, head_major=head_major)
            ref, var = plan_contiguous(p)
            assert ref[0] == 0 and plan(p, pg) == ref
            assert L.tfa_fwd_varlen_paged_variant(C.byref(p), C.byref(pg)) == var and var in (30, 32)
            assert L.tfa_fwd_varlen_paged_rounding_rule(C.byref(p), C.byref(pg)) == _lib.RULE_LAZY
    for v in (30, 32):
        _lib.set_variant(v)
        try:
            assert L.tfa_fwd_varlen_paged_variant(C.byref(p), C.byref(pg)) == v
        finally:
            _lib.set_variant(-1)


def test_pool_of_any_size_and_a_table_shorter_than_max_seqlen_k():
    """No TFA_ERR_STRIDE for K / V: a pool far beyond 4 GiB plans (page bases are 64-bit pointer arithmetic, a descriptor covers one tile) — also where the
    contiguous call refuses the same max_seqlen_k for its one descriptor per sequence; a table row shorter than max_seqlen_k is fine (the length is clamped)."""
    p, pg = params(B=2, H=8, Hk=8, D=128, max_q=1024, max_k=1 << 21, total_q=2048, page=256, num_pages=1 << 22, max_blocks=1 << 13)
    assert plan(p, pg)[0] == 0
    assert plan_contiguous(p)[0][0] == CODES["TFA_ERR_STRIDE"]
    p, pg = params(max_k=8192, max_blocks=3)
    assert plan(p, pg)[0] == 0


def test_refusal_codes():
    L = _lib.lib()
    p, pg = params()
    assert plan(p, pg)[0] == 0
    assert plan(p, None)[0] == CODES["TFA_ERR_NULL"]
    assert L.tfa_fwd_varlen_paged(C.byref(p), None, None) == CODES["TFA_ERR_NULL"]
    assert L.tfa_fwd_varlen_paged(None, C.byref(pg), None) == CODES["TFA_ERR_NULL"]
    assert L.tfa_fwd_varlen_paged_variant(C.byref(p), None) == CODES["TFA_ERR_NULL"]
    assert L.tfa_fwd_varlen_paged_rounding_rule(C.byref(p), None) == CODES["TFA_ERR_NULL"]
    p, pg = params()
    pg.block_table = None
    assert plan(p, pg)[0] == CODES["TFA_ERR_NULL"]
    for field in ("q", "k", "v", "out", "cu_seqlens_q", "cu_seqlens_k"):
        p, pg = params()
        setattr(p, field, None)
        assert plan(p, pg)[0] == CODES["TFA_ERR_NULL"], field
    for page in (0, -64, 32, 96, 100):
        assert plan(*params(page=page))[0] == CODES["TFA_ERR_SHAPE"], page
    for kw in ({"max_blocks": 0}, {"max_blocks": -1}, {"num_pages": 0}, {"num_pages": -3}, {"B": 0}, {"H": 12}, {"max_q": 0}, {"max_k": 0}, {"total_q": 0}):
        assert plan(*params(**kw))[0] == CODES["TFA_ERR_SHAPE"], kw
    p, pg = params()
    p.flags = 1
    assert plan(p, pg)[0] == CODES["TFA_ERR_SHAPE"]
    p, pg = params()
    pg.reserved_ = 1
    assert plan(p, pg)[0] == CODES["TFA_ERR_SHAPE"]
    for D in (0, 4, 12, 136, 256):
        assert plan(*params(D=D))[0] == CODES["TFA_ERR_HEAD_DIM"], D
    assert plan(*params(dtype=_lib.TFA_F32))[0] == CODES["TFA_ERR_DTYPE"]
    p, pg = params()
    pg.block_table = ADDR + 2
    assert plan(p, pg)[0] == CODES["TFA_ERR_ALIGN"]
    for field, val in (("table_stride", -1), ("k_page_stride", -8), ("v_page_stride", 4)):
        p, pg = params()
        setattr(pg, field, val)
        assert plan(p, pg)[0] == CODES["TFA_ERR_STRIDE"], field
    p, pg = params()
    p.k_stride[1] = 64            # rows that overlap (row stride below the head dim)
    assert plan(p, pg)[0] == CODES["TFA_ERR_STRIDE"]
    _lib.set_variant(17)
    try:
        assert plan(*params())[0] == CODES["TFA_ERR_VARIANT"]
    finally:
        _lib.set_variant(-1)
    # total_k is ignored
    p, pg = params()
    p.total_k = -5
    assert plan(p, pg)[0] == 0


# ---- the Python wrapper against a counting stand-in for the library ------------------------------------------------------------------

class _CountingLib:
    """A stand-in for the loaded library object: records every call and answers TFA_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a):
            self.calls.append((name, a))
            return 0
        return f


class _FakeCuda:
    """torch.cuda as ops.py uses it around a launch (current device / stream), without a device."""

    class _Stream:
        cuda_stream = 0

    class device:
        def __init__(self, d):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

    @staticmethod
    def current_stream():
        return _FakeCuda._Stream()


def _meta(*shape, dtype=torch.bfloat16):
    return torch.empty(shape, dtype=dtype, device="meta")


@pytest.fixture
def stub(monkeypatch):
    fake = _CountingLib()
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    monkeypatch.setattr(ops.torch, "cuda", _FakeCuda)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(torch.Tensor, "data_ptr", lambda self: ADDR + 16 * (id(self) % 4096))
    return fake


def test_wrapper_fills_the_structs_from_a_permuted_view_pool(stub):
    import tiny_flash_attention_amd as tfa

    B, tq, H, Hk, D, page, nb, mb = 3, 700, 8, 2, 128, 128, 40, 12
    q = _meta(tq, H, D, dtype=torch.float16)
    kp = _meta(nb, Hk, page, D, dtype=torch.float16).permute(0, 2, 1, 3)          # (num_pages, Hk, page_size, D) memory, passed as (num_pages, page_size, Hk, D)
    vp = _meta(2 * nb, page, Hk, D, dtype=torch.float16)[::2]                       # v: every second page of a larger pool
    bt = _meta(B, 16, dtype=torch.int32)[:, :mb]                                    # rows 16 entries apart
    cq, ck = _meta(B + 1, dtype=torch.int32), _meta(B + 1, dtype=torch.int32)
    out = tfa.flash_attn_varlen_func(q, kp, vp, cq, ck, 300, 1500, 0.0, 0.5, True, block_table=bt)
    assert [c[0] for c in stub.calls] == ["tfa_fwd_varlen_paged"]
    pref, pgref, stream = stub.calls[0][1]
    p, pg = pref._obj, pgref._obj
    assert (p.B, p.H, p.Hk, p.D, p.max_seqlen_q, p.max_seqlen_k, p.total_q) == (B, H, Hk, D, 300, 1500, tq)
    assert (p.q, p.k, p.v, p.cu_seqlens_q, p.cu_seqlens_k) == (q.data_ptr(), kp.data_ptr(), vp.data_ptr(), cq.data_ptr(), ck.data_ptr())
    assert p.lse is None and p.flags == 0 and p.reserved_ == 0
    assert list(p.q_stride) == [D, H * D] and list(p.o_stride) == [D, H * D]
    assert list(p.k_stride) == [page * D, D]                                        # head, row of the permuted view
    assert list(p.v_stride) == [D, Hk * D]
    assert (pg.block_table, pg.table_stride, pg.max_blocks, pg.page_size, pg.num_pages, pg.reserved_) == (bt.data_ptr(), 16, mb, page, nb, 0)
    assert (pg.k_page_stride, pg.v_page_stride) == (Hk * page * D, 2 * page * Hk * D)
    assert p.dtype == _lib.TFA_F16 and p.out_dtype == _lib.TFA_F16 and p.is_causal == 1 and p.softmax_scale == 0.5
    assert tuple(out.shape) == (tq, H, D) and out.dtype == torch.float16
    # ops level: lse and an fp32 out; a (-1, 0) window is the causal call, (-1, -1) the full one
    stub.calls.clear()
    out, lse = ops.flash_attn_varlen_fwd(q, kp, vp, cq, ck, 300, 1500, False, None, out_f32=True, window_size=(-1, 0), block_table=bt)
    p = stub.calls[0][1][0]._obj
    assert [c[0] for c in stub.calls] == ["tfa_fwd_varlen_paged"] and p.is_causal == 1 and p.out_dtype == _lib.TFA_F32 and p.lse == lse.data_ptr()
    assert tuple(lse.shape) == (H, tq) and out.dtype == torch.float32 and abs(p.softmax_scale - 1.0 / 128 ** 0.5) < 1e-7
    stub.calls.clear()
    ops.flash_attn_varlen_fwd(q, kp, vp, cq, ck, 300, 1500, False, None, window_size=(-1, -1), block_table=bt)
    assert stub.calls[0][1][0]._obj.is_causal == 0


def test_wrapper_refuses_by_name_before_any_call(stub):
    import tiny_flash_attention_amd as tfa

    B, H, Hk, D = 2, 8, 2, 64
    q, kp = _meta(100, H, D), _meta(9, 64, Hk, D)
    cq = _meta(B + 1, dtype=torch.int32)
    bt = _meta(B, 4, dtype=torch.int32)

    def f(q=q, k=kp, v=kp, bt=bt, **kw):
        return tfa.flash_attn_varlen_func(q, k, v, cq, cq, 64, 256, block_table=bt, **kw)

    with pytest.raises(ValueError, match="window_size"):
        f(window_size=(16, 0))
    with pytest.raises(ValueError, match="window_size"):
        f(window_size=(-1, 3))
    with pytest.raises(ValueError, match="softcap"):
        f(softcap=30.0)
    with pytest.raises(ValueError, match="alibi_slopes"):
        f(alibi_slopes=_meta(H, dtype=torch.float32))
    with pytest.raises(NotImplementedError, match="dropout"):
        f(dropout_p=0.1)
    with pytest.raises(TypeError, match="fp8"):
        f(k=_meta(9, 64, Hk, D, dtype=torch.float8_e4m3fn), v=_meta(9, 64, Hk, D, dtype=torch.float8_e4m3fn))
    with pytest.raises(TypeError, match="dtype"):
        f(k=_meta(9, 64, Hk, D, dtype=torch.float16), v=_meta(9, 64, Hk, D, dtype=torch.float16))
    with pytest.raises(TypeError):
        f(q=_meta(100, H, D, dtype=torch.float32), k=_meta(9, 64, Hk, D, dtype=torch.float32), v=_meta(9, 64, Hk, D, dtype=torch.float32))
    with pytest.raises(ValueError, match="4-D"):
        f(k=_meta(576, Hk, D), v=_meta(576, Hk, D))
    with pytest.raises(ValueError, match="multiple of 64"):
        f(k=_meta(9, 48, Hk, D), v=_meta(9, 48, Hk, D))
    with pytest.raises(ValueError, match="head dims up to 128"):
        f(q=_meta(100, H, 256), k=_meta(9, 64, Hk, 256), v=_meta(9, 64, Hk, 256))
    with pytest.raises(ValueError, match="block_table"):
        f(bt=_meta(B, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="block_table"):
        f(bt=_meta(B + 1, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="block_table"):
        f(bt=_meta(4, B, dtype=torch.int32).t())                                     # no unit stride along max_blocks
    with pytest.raises(ValueError, match="block_table"):
        f(bt=_meta(B * 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="unit stride"):
        f(k=_meta(9, 64, Hk, 2 * D)[..., ::2], v=_meta(9, 64, Hk, 2 * D)[..., ::2])
    with pytest.raises(ValueError, match="K/V heads"):
        f(k=_meta(9, 64, 3, D), v=_meta(9, 64, 3, D))
    qg = _meta(100, H, D).requires_grad_(True)
    with pytest.raises(RuntimeError, match="not differentiable"):
        f(q=qg)
    assert stub.calls == []
    with torch.no_grad():
        f(q=qg)
    assert [c[0] for c in stub.calls] == ["tfa_fwd_varlen_paged"]


def test_without_block_table_the_call_is_todays(stub):
    """block_table=None (given or not): exactly the library calls the function made before the keyword existed, with the same parameter block."""
    import tiny_flash_attention_amd as tfa

    B, H, Hk, D = 3, 8, 2, 64
    q, k, v = _meta(500, H, D), _meta(900, Hk, D), _meta(900, Hk, D)
    cq, ck = _meta(B + 1, dtype=torch.int32), _meta(B + 1, dtype=torch.int32)
    blocks = []
    for kw in ({}, {"block_table": None}):
        for args, name in ((dict(causal=True), "tfa_fwd_varlen"), (dict(window_size=(32, 0)), "tfa_fwd_varlen_local"),
                           (dict(softcap=20.0), "tfa_fwd_varlen_softcap"), (dict(alibi_slopes=_meta(H, dtype=torch.float32)), "tfa_fwd_varlen_alibi")):
            stub.calls.clear()
            tfa.flash_attn_varlen_func(q, k, v, cq, ck, 200, 400, **args, **kw)
            assert [c[0] for c in stub.calls] == [name]
            p = stub.calls[0][1][0]._obj
            blocks.append((name, stub.calls[0][1][1:-1] if name != "tfa_fwd_varlen_alibi" else stub.calls[0][1][2:-1],
                           (p.q, p.k, p.v, p.B, p.H, p.Hk, p.D, p.max_seqlen_q, p.max_seqlen_k, p.total_q, p.total_k, list(p.q_stride), list(p.k_stride),
                            list(p.v_stride), list(p.o_stride), p.is_causal, p.dtype, p.out_dtype, p.softmax_scale)))
    assert blocks[:4] == blocks[4:]
    assert blocks[0][2][10] == 900 and blocks[0][2][12] == [D, Hk * D]
    # the autograd route keeps its call too
    stub.calls.clear()
    qg = _meta(500, H, D).requires_grad_(True)
    tfa.flash_attn_varlen_func(qg, k, v, cq, ck, 200, 400, causal=True, block_table=None)
    assert [c[0] for c in stub.calls] == ["tfa_fwd_varlen"]
