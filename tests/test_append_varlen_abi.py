"""CPU tests of the packed append (include/tfa.h: tfa_kvcache_append_varlen, _plan) and of the Python wrapper ``kvcache_append_varlen``: symbols, struct size,
plans of paged and contiguous caches, one case per refusal code, and the wrapper's host-side behaviour against a counting stand-in for the library.
No GPU: plans never launch, refused calls return before any launch, cu_seqlens / cache_seqlens / the block table are never read on the host."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest
import torch

from tiny_flash_attention_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDR = 0x10000          # a 16-byte aligned stand-in for device pointers (plans never dereference them)
CODES = {"TFA_ERR_NULL": -1, "TFA_ERR_DTYPE": -2, "TFA_ERR_HEAD_DIM": -3, "TFA_ERR_SHAPE": -4, "TFA_ERR_STRIDE": -5, "TFA_ERR_ALIGN": -6}
SYMBOLS = ("tfa_kvcache_append_varlen", "tfa_kvcache_append_varlen_plan")


def params(B=4, total=74, Hk=2, D=64, page=64, max_blocks=4, num_pages=20, cap=256, rd=0, ro=512, dtype=_lib.TFA_BF16, cs_dtype=None, interleaved=False):
    """A tfa_kvcache_append_varlen_params: packed contiguous k / v, a paged pool (page > 0) or a contiguous (B, cap, Hk, D) cache, tables when rd > 0."""
    p = _lib.TfaKvcacheAppendVarlenParams()
    p.k, p.v, p.k_cache, p.v_cache, p.cu_seqlens, p.cache_seqlens = ADDR, 2 * ADDR, 3 * ADDR, 4 * ADDR, 5 * ADDR, 6 * ADDR
    p.B, p.total_new, p.Hk, p.D = B, total, Hk, D
    for name in ("k_stride", "v_stride"):
        arr = getattr(p, name)
        arr[0], arr[1] = D, Hk * D
    rows = page if page else cap
    for name in ("kc_stride", "vc_stride"):
        arr = getattr(p, name)
        arr[0], arr[1], arr[2] = rows * Hk * D, D, Hk * D
    if page:
        p.block_table = 7 * ADDR
        p.page_size, p.num_pages, p.capacity, p.block_table_stride = page, num_pages, max_blocks * page, max_blocks
    else:
        p.capacity = cap
    if rd:
        p.rotary_cos, p.rotary_sin = 8 * ADDR, 9 * ADDR
        p.rotary_dim, p.seqlen_ro, p.cos_stride, p.sin_stride = rd, ro, rd // 2, rd // 2
        p.rotary_interleaved = 1 if interleaved else 0
        p.cs_dtype = dtype if cs_dtype is None else cs_dtype
    p.dtype = dtype
    return p


def plan(p):
    g, b = C.c_int(), C.c_int()
    return _lib.lib().tfa_kvcache_append_varlen_plan(C.byref(p), C.byref(g), C.byref(b)), g.value, b.value


def test_symbols_exported_and_version():
    L = _lib.lib()
    for s in SYMBOLS:
        assert s in _lib.SYMBOLS
        getattr(L, s)
    assert L.tfa_version() == 111


def test_struct_size_matches_the_header():
    src = '#include <stdio.h>\n#include "tfa.h"\nint main(void) { printf("%zu", sizeof(tfa_kvcache_append_varlen_params)); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.check_call(["cc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        assert int(subprocess.check_output([exe]).decode()) == C.sizeof(_lib.TfaKvcacheAppendVarlenParams)


@pytest.mark.parametrize("D", [64, 40, 128, 8])
@pytest.mark.parametrize("page", [0, 64, 128, 256])
def test_plan_is_one_thread_per_row_head_and_chunk(D, page):
    for total, Hk in ((74, 2), (1, 1), (4096, 8)):
        for dtype in (_lib.TFA_BF16, _lib.TFA_F16):
            want = (0, -(-total * Hk * (D // 8) // 256), 256)
            assert plan(params(total=total, Hk=Hk, D=D, page=page, dtype=dtype)) == want
            if D >= 16:
                for cs in (dtype, _lib.TFA_F32):
                    for il in (False, True):
                        assert plan(params(total=total, Hk=Hk, D=D, page=page, dtype=dtype, rd=16, cs_dtype=cs, interleaved=il)) == want


@pytest.mark.parametrize("field", ["k", "v", "k_cache", "v_cache", "cu_seqlens", "cache_seqlens", "rotary_cos", "rotary_sin"])
def test_refusal_null(field):
    p = params(rd=32)
    setattr(p, field, None)
    assert plan(p)[0] == CODES["TFA_ERR_NULL"]
    assert _lib.lib().tfa_kvcache_append_varlen(C.byref(p), None) == CODES["TFA_ERR_NULL"]


def test_refusal_null_params():
    assert _lib.lib().tfa_kvcache_append_varlen_plan(None, None, None) == CODES["TFA_ERR_NULL"]
    assert _lib.lib().tfa_kvcache_append_varlen(None, None) == CODES["TFA_ERR_NULL"]


def test_refusal_dtype():
    for dtype in (_lib.TFA_F32, 7, -1):
        assert plan(params(dtype=dtype))[0] == CODES["TFA_ERR_DTYPE"]
    assert plan(params(rd=32, cs_dtype=_lib.TFA_F16))[0] == CODES["TFA_ERR_DTYPE"]        # f16 tables for bf16 rows


@pytest.mark.parametrize("D,rd", [(0, 0), (4, 0), (12, 0), (136, 0), (256, 0), (64, 8), (64, 24), (64, 80), (40, 48)])
def test_refusal_head_dim(D, rd):
    p = params(rd=16)
    p.D, p.rotary_dim = D, rd if rd else 16
    assert plan(p)[0] == CODES["TFA_ERR_HEAD_DIM"]


@pytest.mark.parametrize("kw", [dict(B=0), dict(total=0), dict(Hk=0), dict(page=0, cap=0), dict(total=-5)])
def test_refusal_shapes(kw):
    assert plan(params(**kw))[0] == CODES["TFA_ERR_SHAPE"]


@pytest.mark.parametrize("page", [-64, 1, 32, 96, 100, 65])
def test_refusal_page_size(page):
    p = params()
    p.page_size = page
    assert plan(p)[0] == CODES["TFA_ERR_SHAPE"]


def test_refusal_paged_geometry_tables_and_reserved():
    p = params()
    p.capacity = 256 + 32                           # not whole pages
    assert plan(p)[0] == CODES["TFA_ERR_SHAPE"]
    p = params()
    p.num_pages = 0
    assert plan(p)[0] == CODES["TFA_ERR_SHAPE"]
    p = params()
    p.reserved_ = 1
    assert plan(p)[0] == CODES["TFA_ERR_SHAPE"]
    assert plan(params(rd=32, ro=0))[0] == CODES["TFA_ERR_SHAPE"]
    p = params(rd=32)
    p.rotary_interleaved = 2
    assert plan(p)[0] == CODES["TFA_ERR_SHAPE"]
    p = params()
    p.block_table_stride = 3                        # rows of the table overlap
    assert plan(p)[0] == CODES["TFA_ERR_STRIDE"]


@pytest.mark.parametrize("name,n", [("k_stride", 2), ("v_stride", 2), ("kc_stride", 3), ("vc_stride", 3)])
def test_refusal_strides(name, n):
    for i in range(n):
        p = params()
        getattr(p, name)[i] = -128
        assert plan(p)[0] == CODES["TFA_ERR_STRIDE"]
        p = params()
        getattr(p, name)[i] = 132                   # 264 bytes: chunks no longer 16-byte aligned
        assert plan(p)[0] == CODES["TFA_ERR_STRIDE"]
    p = params()
    getattr(p, name)[n - 1] = 32                    # rows overlap (D = 64)
    assert plan(p)[0] == CODES["TFA_ERR_STRIDE"]
    p = params(rd=32)
    p.cos_stride = 8                                # table rows overlap
    assert plan(p)[0] == CODES["TFA_ERR_STRIDE"]


@pytest.mark.parametrize("field,off", [("k", 8), ("v", 8), ("k_cache", 8), ("v_cache", 8), ("rotary_cos", 8), ("rotary_sin", 8), ("cu_seqlens", 2),
                                       ("cache_seqlens", 2), ("block_table", 2)])
def test_refusal_alignment(field, off):
    p = params(rd=32)
    setattr(p, field, getattr(p, field) + off)
    assert plan(p)[0] == CODES["TFA_ERR_ALIGN"]


def test_header_still_compiles_as_plain_c():
    src = ('#include "tfa.h"\nint main(void) { tfa_kvcache_append_varlen_params p; (void)p; (void)tfa_kvcache_append_varlen; '
           '(void)tfa_kvcache_append_varlen_plan; return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "h.c")
        open(c, "w").write(src)
        subprocess.check_call(["cc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", c, "-o", os.path.join(d, "h.o")])


# ---- Python: kvcache_append_varlen against the counting stand-in -----------------------------------------------------------------------------
class _CountingLib:
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


def _ptr(t):
    """A stand-in address: one 1 MiB region per storage, the view's offset inside it — so views of one buffer differ by their offsets, as on a device."""
    return ADDR * 16 * (1 + id(t.untyped_storage()) % 4096) + t.storage_offset() * t.element_size()


@pytest.fixture
def stub(monkeypatch):
    fake = _CountingLib()
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    monkeypatch.setattr(ops.torch, "cuda", _FakeCuda)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(torch.Tensor, "data_ptr", _ptr)
    return fake


def _i32(*shape):
    return _meta(*shape, dtype=torch.int32)


def test_wrapper_is_exported():
    import tiny_flash_attention_amd as tfa

    assert tfa.kvcache_append_varlen is ops.kvcache_append_varlen and "kvcache_append_varlen" in tfa.__all__


def test_wrapper_paged_call_with_sliced_projection_and_permuted_pool(stub):
    total, H, Hk, D, B, page, nb, mb = 74, 8, 2, 64, 4, 128, 10, 3
    qkv = _meta(total, H + 2 * Hk, D)
    k, v = qkv[:, H:H + Hk], qkv[:, H + Hk:]
    kc = _meta(nb, Hk, page, D).transpose(1, 2)                              # a (num_pages, Hk, page_size, D) pool viewed as (num_pages, page_size, Hk, D)
    vc = _meta(nb, page, Hk, D)
    bt = _i32(B, 8)[:, :mb]
    cu, lens = _i32(B + 1), _i32(B)
    assert ops.kvcache_append_varlen(k, v, kc, vc, cu, lens, bt) is None
    assert [c[0] for c in stub.calls] == ["tfa_kvcache_append_varlen"]
    p = stub.calls[0][1][0]._obj
    assert (p.k, p.v, p.k_cache, p.v_cache) == (_ptr(k), _ptr(v), _ptr(kc), _ptr(vc)) and p.v == p.k + Hk * D * 2
    assert (p.cu_seqlens, p.cache_seqlens, p.block_table) == (_ptr(cu), _ptr(lens), _ptr(bt))
    assert (p.B, p.total_new, p.Hk, p.D, p.capacity, p.page_size, p.num_pages, p.block_table_stride) == (B, total, Hk, D, mb * page, page, nb, 8)
    row = (H + 2 * Hk) * D
    assert list(p.k_stride) == [D, row] == list(p.v_stride)
    assert list(p.kc_stride) == [Hk * page * D, page * D, D] and list(p.vc_stride) == [page * Hk * D, D, Hk * D]
    assert p.dtype == _lib.TFA_BF16 and p.rotary_cos is None and p.rotary_sin is None and p.reserved_ == 0


def test_wrapper_contiguous_cache_with_rotary_tables(stub):
    total, Hk, D, B, cap, rd, ro = 9, 2, 128, 3, 512, 32, 600
    k, v = _meta(total, Hk, D, dtype=torch.float16), _meta(total, Hk, D, dtype=torch.float16)
    kc, vc = _meta(B, cap, Hk, D, dtype=torch.float16), _meta(B, 2 * cap, Hk, D, dtype=torch.float16)[:, :cap]
    cos, sin = _meta(ro, rd // 2, dtype=torch.float32), _meta(ro, rd // 2, dtype=torch.float32)
    ops.kvcache_append_varlen(k, v, kc, vc, _i32(B + 1), _i32(B), rotary_cos=cos, rotary_sin=sin, rotary_interleaved=True)
    p = stub.calls[0][1][0]._obj
    assert p.block_table is None and p.capacity == cap
    assert list(p.kc_stride) == [cap * Hk * D, D, Hk * D] and list(p.vc_stride) == [2 * cap * Hk * D, D, Hk * D]
    assert (p.rotary_cos, p.rotary_sin, p.cos_stride, p.sin_stride) == (_ptr(cos), _ptr(sin), rd // 2, rd // 2)
    assert (p.rotary_dim, p.seqlen_ro, p.rotary_interleaved, p.dtype, p.cs_dtype) == (rd, ro, 1, _lib.TFA_F16, _lib.TFA_F32)


def test_wrapper_refuses_by_name_before_any_call(stub):
    f = ops.kvcache_append_varlen
    B, total, Hk, D = 2, 6, 2, 64
    k, v, kc, vc = _meta(total, Hk, D), _meta(total, Hk, D), _meta(5, 64, Hk, D), _meta(5, 64, Hk, D)
    cu, lens, bt = _i32(B + 1), _i32(B), _i32(B, 3)
    for i in range(6):
        a = [k, v, kc, vc, cu, lens]
        a[i] = None
        with pytest.raises(TypeError, match="must be a tensor"):
            f(*a, bt)
    with pytest.raises(TypeError, match="float16 or bfloat16"):
        f(_meta(total, Hk, D, dtype=torch.float32), v, kc, vc, cu, lens, bt)
    k8 = _meta(5, 64, Hk, D, dtype=torch.float8_e4m3fn)
    with pytest.raises(TypeError, match="fp8 caches are not served"):
        f(k, v, k8, k8, cu, lens, bt)
    with pytest.raises(TypeError, match="k's dtype"):
        f(k, v, kc.to(torch.float16), vc.to(torch.float16), cu, lens, bt)
    with pytest.raises(ValueError, match="3-D"):
        f(_meta(1, total, Hk, D), v, kc, vc, cu, lens, bt)
    with pytest.raises(ValueError, match="4-D"):
        f(k, v, _meta(64, Hk, D), vc, cu, lens, bt)
    with pytest.raises(ValueError, match="one non-empty shape"):
        f(k, _meta(total + 1, Hk, D), kc, vc, cu, lens, bt)
    with pytest.raises(ValueError, match="one shape"):
        f(k, v, kc, _meta(5, 64, Hk + 1, D), cu, lens, bt)
    with pytest.raises(ValueError, match="multiple of 64"):
        f(k, v, _meta(5, 48, Hk, D), _meta(5, 48, Hk, D), cu, lens, bt)
    with pytest.raises(ValueError, match="multiple of 8 up to 128"):
        f(_meta(total, Hk, 256), _meta(total, Hk, 256), _meta(5, 64, Hk, 256), _meta(5, 64, Hk, 256), cu, lens, bt)
    with pytest.raises(ValueError, match="unit stride"):
        f(_meta(total, D, Hk).transpose(1, 2), v, kc, vc, cu, lens, bt)
    for bad in (_meta(B + 1, dtype=torch.int64), _i32(B + 1, 1), _i32(1), _i32(2 * B + 2)[::2], torch.empty(B + 1, dtype=torch.int32)):
        with pytest.raises(ValueError, match="cu_seqlens"):
            f(k, v, kc, vc, bad, lens, bt)
    for bad in (_meta(B, dtype=torch.int64), _i32(B + 1), _i32(B, 1), _i32(2 * B)[::2], torch.empty(B, dtype=torch.int32)):
        with pytest.raises(ValueError, match="cache_seqlens"):
            f(k, v, kc, vc, cu, bad, bt)
    for bad in (_meta(B, 3, dtype=torch.int64), _i32(B + 1, 3), _i32(3), _i32(3, B).t(), torch.empty((B, 3), dtype=torch.int32), [[0, 1, 2]] * B):
        with pytest.raises(ValueError, match="block_table"):
            f(k, v, kc, vc, cu, lens, bad)
    with pytest.raises(ValueError, match="one slice per sequence"):
        f(k, v, kc, vc, cu, lens)                                           # five slices, two sequences
    cos = _meta(32, 16)
    with pytest.raises(ValueError, match="together"):
        f(k, v, kc, vc, cu, lens, bt, rotary_cos=cos)
    with pytest.raises(ValueError, match="multiple of 16"):
        f(k, v, kc, vc, cu, lens, bt, rotary_cos=_meta(32, 12), rotary_sin=_meta(32, 12))
    with pytest.raises(ValueError, match="exceed the head dim"):
        f(k, v, kc, vc, cu, lens, bt, rotary_cos=_meta(32, 40), rotary_sin=_meta(32, 40))
    with pytest.raises(ValueError, match="rotary_cos and rotary_sin must have one shape and dtype"):
        f(k, v, kc, vc, cu, lens, bt, rotary_cos=cos, rotary_sin=_meta(32, 16, dtype=torch.float32))
    with pytest.raises(TypeError, match="rotary_sin must be a tensor"):
        f(k, v, kc, vc, cu, lens, bt, rotary_cos=cos, rotary_sin=1.0)
    with pytest.raises(RuntimeError, match="not differentiable"):
        f(_meta(total, Hk, D).requires_grad_(True), v, kc, vc, cu, lens, bt)
    assert stub.calls == []
    f(k, v, kc, vc, cu, lens, bt, rotary_cos=cos, rotary_sin=cos)
    assert len(stub.calls) == 1
