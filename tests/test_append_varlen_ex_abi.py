"""CPU tests of the packed append into an e4m3 cache and / or with q rotated in the launch (include/tfa.h: tfa_kvcache_append_varlen_ex, _plan) and of the three
keywords it adds to ``kvcache_append_varlen`` (q=, k_descale=, v_descale=): symbols, struct size, plans of paged and contiguous caches, one case per refusal code,
and the wrapper's host-side behaviour against a counting stand-in for the library.  No GPU: plans never launch, refused calls return before any launch, nothing
is read on the host."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest
import torch

from tiny_flash_attention_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDR = 0x10000          # a 16-byte aligned stand-in for device pointers (plans never dereference them)
CODES = {"TFA_OK": 0, "TFA_ERR_NULL": -1, "TFA_ERR_DTYPE": -2, "TFA_ERR_HEAD_DIM": -3, "TFA_ERR_SHAPE": -4, "TFA_ERR_STRIDE": -5, "TFA_ERR_ALIGN": -6}
SYMBOLS = ("tfa_kvcache_append_varlen_ex", "tfa_kvcache_append_varlen_ex_plan")
E4M3 = torch.float8_e4m3fn


def params(B=4, total=74, Hk=2, D=64, page=64, max_blocks=4, num_pages=20, cap=256, rd=0, ro=512, dtype=_lib.TFA_BF16, cs_dtype=None, interleaved=False):
    """tests/test_append_varlen_abi.py's: packed contiguous k / v, a paged pool (page > 0) or a contiguous (B, cap, Hk, D) cache, tables when rd > 0.  The cache
    strides are in cache elements: the same numbers serve a 16-bit and an e4m3 cache (there they count bytes)."""
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


def fp8(Hk=2, broadcast=False):
    q8 = _lib.TfaKvcacheFp8()
    q8.k_descale, q8.v_descale, q8.format = 10 * ADDR, 11 * ADDR, _lib.TFA_KV_E4M3
    for arr in (q8.k_descale_stride, q8.v_descale_stride):
        arr[0], arr[1] = (0, 0) if broadcast else (Hk, 1)
    return q8


def rotq(H=8, D=64, heads_in_row=None):
    rq = _lib.TfaAppendQ()
    rq.q, rq.H = 12 * ADDR, H
    rq.q_stride[0], rq.q_stride[1] = D, (heads_in_row or H) * D
    return rq


def plan(p, q8=None, rq=None):
    g, b = C.c_int(), C.c_int()
    st = _lib.lib().tfa_kvcache_append_varlen_ex_plan(C.byref(p), C.byref(q8) if q8 is not None else None, C.byref(rq) if rq is not None else None,
                                                      C.byref(g), C.byref(b))
    return st, g.value, b.value


def code(p, q8=None, rq=None):
    """The plan's status, and the launching entry point's: a refused call returns before any launch."""
    st = plan(p, q8, rq)[0]
    if st != 0:
        assert _lib.lib().tfa_kvcache_append_varlen_ex(C.byref(p), C.byref(q8) if q8 is not None else None, C.byref(rq) if rq is not None else None, None) == st
    return st


def old_plan(p):
    g, b = C.c_int(), C.c_int()
    return _lib.lib().tfa_kvcache_append_varlen_plan(C.byref(p), C.byref(g), C.byref(b)), g.value, b.value


def test_symbols_exported_and_version_stays():
    L = _lib.lib()
    for s in SYMBOLS:
        assert s in _lib.SYMBOLS
        getattr(L, s)
    assert L.tfa_version() == 111


def test_struct_size_matches_the_header_and_the_header_compiles_as_plain_c():
    src = ('#include <stdio.h>\n#include "tfa.h"\nint main(void) { (void)tfa_kvcache_append_varlen_ex; (void)tfa_kvcache_append_varlen_ex_plan; '
           'printf("%zu %zu", sizeof(tfa_append_q), sizeof(tfa_kvcache_append_varlen_params)); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.check_call(["cc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        assert [int(x) for x in subprocess.check_output([exe]).decode().split()] == [C.sizeof(_lib.TfaAppendQ), C.sizeof(_lib.TfaKvcacheAppendVarlenParams)]


# ---- plans ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page", [0, 64, 256])
@pytest.mark.parametrize("D", [16, 64, 128])
def test_plan_fp8_only_is_the_appends_geometry(D, page):
    for total, Hk in ((74, 2), (1, 1), (4096, 8)):
        for dtype in (_lib.TFA_BF16, _lib.TFA_F16):
            want = (0, -(-total * Hk * (D // 8) // 256), 256)
            assert plan(params(total=total, Hk=Hk, D=D, page=page, dtype=dtype), fp8(Hk)) == want
            assert plan(params(total=total, Hk=Hk, D=D, page=page, dtype=dtype), fp8(Hk, broadcast=True)) == want
            for cs in (dtype, _lib.TFA_F32):
                for il in (False, True):
                    assert plan(params(total=total, Hk=Hk, D=D, page=page, dtype=dtype, rd=16, cs_dtype=cs, interleaved=il), fp8(Hk)) == want


@pytest.mark.parametrize("page", [0, 64, 256])
@pytest.mark.parametrize("with_fp8", [False, True])
def test_plan_with_q_adds_one_thread_per_item_of_the_rotated_part(with_fp8, page):
    for total, Hk, H, D, rd in ((74, 2, 8, 64, 32), (1, 1, 1, 16, 16), (4096, 8, 32, 128, 128), (9, 2, 2, 128, 64)):
        for il in (False, True):
            items = rd // 8 if il else rd // 16
            want = (0, -(-(total * Hk * (D // 8) + total * H * items) // 256), 256)
            p = params(total=total, Hk=Hk, D=D, page=page, rd=rd, interleaved=il)
            assert plan(p, fp8(Hk) if with_fp8 else None, rotq(H, D)) == want
            assert plan(p, fp8(Hk) if with_fp8 else None, rotq(H, D, heads_in_row=H + 2 * Hk)) == want        # a slice of a packed projection


@pytest.mark.parametrize("page", [0, 64, 128])
def test_plan_without_companions_is_the_old_entry_points(page):
    for D in (64, 40, 8, 128):
        for rd in (0, 16) if D >= 16 else (0,):
            p = params(D=D, page=page, rd=rd)
            assert plan(p) == old_plan(p) and plan(p)[0] == 0
    p = params(D=4)
    assert plan(p) == old_plan(p) and plan(p)[0] == CODES["TFA_ERR_HEAD_DIM"]


# ---- refusals: what the plain entry point refuses -------------------------------------------------------------------------------------------------
def test_refuses_what_the_plain_append_refuses():
    for q8, rq in ((fp8(), None), (None, rotq()), (fp8(), rotq())):
        assert _lib.lib().tfa_kvcache_append_varlen_ex_plan(None, None if q8 is None else C.byref(q8), None if rq is None else C.byref(rq), None, None) == CODES["TFA_ERR_NULL"]
        for field in ("k", "v", "k_cache", "v_cache", "cu_seqlens", "cache_seqlens", "rotary_sin"):
            p = params(rd=32)
            setattr(p, field, None)
            assert code(p, q8, rq) == CODES["TFA_ERR_NULL"], field
        assert code(params(rd=32, dtype=_lib.TFA_F32), q8, rq) == CODES["TFA_ERR_DTYPE"]
        assert code(params(rd=32, cs_dtype=_lib.TFA_F16), q8, rq) == CODES["TFA_ERR_DTYPE"]
        p = params(rd=32)
        p.D = 256
        assert code(p, q8, rq) == CODES["TFA_ERR_HEAD_DIM"]
        p = params(rd=32)
        p.rotary_dim = 24
        assert code(p, q8, rq) == CODES["TFA_ERR_HEAD_DIM"]
        for kw in (dict(B=0), dict(total=0), dict(Hk=0), dict(page=0, cap=0), dict(ro=0)):
            assert code(params(rd=32, **kw), q8, rq) == CODES["TFA_ERR_SHAPE"], kw
        p = params(rd=32)
        p.page_size = 96
        assert code(p, q8, rq) == CODES["TFA_ERR_SHAPE"]
        p = params(rd=32)
        p.reserved_ = 1
        assert code(p, q8, rq) == CODES["TFA_ERR_SHAPE"]
        p = params(rd=32)
        p.block_table_stride = 3
        assert code(p, q8, rq) == CODES["TFA_ERR_STRIDE"]
        for name, n in (("k_stride", 2), ("v_stride", 2), ("kc_stride", 3), ("vc_stride", 3)):
            for i in range(n):
                p = params(rd=32)
                getattr(p, name)[i] = -128
                assert code(p, q8, rq) == CODES["TFA_ERR_STRIDE"]
            p = params(rd=32)
            getattr(p, name)[n - 1] = 32                 # rows overlap (D = 64)
            assert code(p, q8, rq) == CODES["TFA_ERR_STRIDE"]
        for field, off in (("k", 8), ("v_cache", 8), ("rotary_cos", 8), ("cu_seqlens", 2), ("cache_seqlens", 2), ("block_table", 2)):
            p = params(rd=32)
            setattr(p, field, getattr(p, field) + off)
            assert code(p, q8, rq) == CODES["TFA_ERR_ALIGN"], field


# ---- refusals: from the tfa_kvcache_fp8 -------------------------------------------------------------------------------------------------------------
def test_fp8_refusal_format():
    for fmt in (0, 2, -1):
        q8 = fp8()
        q8.format = fmt
        assert code(params(), q8) == CODES["TFA_ERR_DTYPE"]


def test_fp8_refusal_reserved():
    q8 = fp8()
    q8.reserved_ = 1
    assert code(params(), q8) == CODES["TFA_ERR_SHAPE"]


@pytest.mark.parametrize("D", [8, 24, 40, 120, 136])
def test_fp8_refusal_head_dim(D):
    assert code(params(D=D), fp8()) == CODES["TFA_ERR_HEAD_DIM"]
    if D <= 128:
        assert code(params(D=D)) == 0                    # ... which the 16-bit cache takes


@pytest.mark.parametrize("name", ["kc_stride", "vc_stride"])
def test_fp8_refusal_cache_strides_count_bytes(name):
    for i in range(3):
        p = params()
        getattr(p, name)[i] = 72 if i == 2 else 8        # 16-byte multiples for 2-byte elements (the 16-bit call takes them), not for bytes
        assert code(p, fp8()) == CODES["TFA_ERR_STRIDE"]
        if i != 2:
            assert code(p) == 0


@pytest.mark.parametrize("name", ["k_descale_stride", "v_descale_stride"])
def test_fp8_refusal_negative_descale_stride(name):
    for i in range(2):
        q8 = fp8()
        getattr(q8, name)[i] = -1
        assert code(params(), q8) == CODES["TFA_ERR_STRIDE"]


@pytest.mark.parametrize("field", ["k_descale", "v_descale"])
def test_fp8_refusal_misaligned_descale(field):
    q8 = fp8()
    setattr(q8, field, getattr(q8, field) + 2)
    assert code(params(), q8) == CODES["TFA_ERR_ALIGN"]


# ---- refusals: from the tfa_append_q ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_fp8", [False, True])
def test_q_refusals(with_fp8):
    q8 = fp8() if with_fp8 else None
    rq = rotq()
    rq.q = None
    assert code(params(rd=32), q8, rq) == CODES["TFA_ERR_NULL"]
    assert code(params(rd=0), q8, rotq()) == CODES["TFA_ERR_NULL"]                  # q without tables
    for H in (0, -3):
        assert code(params(rd=32), q8, rotq(H=H, heads_in_row=8)) == CODES["TFA_ERR_SHAPE"]
    rq = rotq()
    rq.reserved_ = 1
    assert code(params(rd=32), q8, rq) == CODES["TFA_ERR_SHAPE"]
    for i in range(2):
        for bad in (-128, 132):                                                       # negative; 264 bytes: chunks no longer 16-byte aligned
            rq = rotq()
            rq.q_stride[i] = bad
            assert code(params(rd=32), q8, rq) == CODES["TFA_ERR_STRIDE"]
    rq = rotq()
    rq.q_stride[1] = 32                                                               # rows overlap (D = 64)
    assert code(params(rd=32), q8, rq) == CODES["TFA_ERR_STRIDE"]
    rq = rotq()
    rq.q += 8
    assert code(params(rd=32), q8, rq) == CODES["TFA_ERR_ALIGN"]
    assert code(params(rd=32), q8, rotq()) == 0


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


def _args(call):
    """(params, tfa_kvcache_fp8 or None, tfa_append_q or None) of a recorded tfa_kvcache_append_varlen_ex call."""
    a = call[1]
    return a[0]._obj, (a[1]._obj if a[1] is not None else None), (a[2]._obj if a[2] is not None else None)


def test_wrapper_fp8_pool_byte_strides_expanded_descales_and_q_slice(stub):
    total, H, Hk, D, B, page, nb, mb = 74, 8, 2, 64, 4, 128, 10, 3
    qkv = _meta(total, 3, H, D)                                                # k / v: slices of a second projection
    q = qkv[:, 0]
    kv = _meta(total, 2 * Hk, D)
    k, v = kv[:, :Hk], kv[:, Hk:]
    kc = _meta(nb, Hk, page, D, dtype=E4M3).transpose(1, 2)                    # a (num_pages, Hk, page_size, D) pool viewed as (num_pages, page_size, Hk, D)
    vc = _meta(nb, page, Hk, D, dtype=E4M3)
    kd = _meta(1, 1, dtype=torch.float32).expand(B, Hk)
    vd = _meta(B, 2 * Hk, dtype=torch.float32)[:, ::2]
    cos, sin = _meta(300, 16, dtype=torch.float32), _meta(300, 16, dtype=torch.float32)
    bt, cu, lens = _i32(B, 8)[:, :mb], _i32(B + 1), _i32(B)
    assert ops.kvcache_append_varlen(k, v, kc, vc, cu, lens, bt, rotary_cos=cos, rotary_sin=sin, q=q, k_descale=kd, v_descale=vd) is None
    assert [c[0] for c in stub.calls] == ["tfa_kvcache_append_varlen_ex"]
    p, q8, rq = _args(stub.calls[0])
    assert (p.k, p.v, p.k_cache, p.v_cache) == (_ptr(k), _ptr(v), _ptr(kc), _ptr(vc))
    assert (p.B, p.total_new, p.Hk, p.D, p.capacity, p.page_size, p.num_pages, p.block_table_stride) == (B, total, Hk, D, mb * page, page, nb, 8)
    assert list(p.k_stride) == [D, 2 * Hk * D] == list(p.v_stride)
    assert list(p.kc_stride) == [Hk * page * D, page * D, D] and list(p.vc_stride) == [page * Hk * D, D, Hk * D]       # bytes: one per element
    assert p.dtype == _lib.TFA_BF16 and p.cs_dtype == _lib.TFA_F32 and (p.rotary_dim, p.seqlen_ro, p.rotary_interleaved) == (32, 300, 0)
    assert (q8.k_descale, q8.v_descale, q8.format, q8.reserved_) == (_ptr(kd), _ptr(vd), _lib.TFA_KV_E4M3, 0)
    assert list(q8.k_descale_stride) == [0, 0] and list(q8.v_descale_stride) == [2 * Hk, 2]
    assert (rq.q, rq.H, rq.reserved_) == (_ptr(q), H, 0) and list(rq.q_stride) == [D, 3 * H * D]
    assert stub.calls[0][1][3].value in (0, None)                                # the current stream


def test_wrapper_fp8_without_q_and_q_without_fp8(stub):
    total, H, Hk, D, B, cap = 9, 4, 2, 128, 3, 512
    k, v = _meta(total, Hk, D, dtype=torch.float16), _meta(total, Hk, D, dtype=torch.float16)
    cu, lens = _i32(B + 1), _i32(B)
    k8, v8 = _meta(B, cap, Hk, D, dtype=E4M3), _meta(B, 2 * cap, Hk, D, dtype=E4M3)[:, :cap]
    kd = vd = _meta(B, Hk, dtype=torch.float32)
    ops.kvcache_append_varlen(k, v, k8, v8, cu, lens, k_descale=kd, v_descale=vd)
    p, q8, rq = _args(stub.calls[0])
    assert stub.calls[0][0] == "tfa_kvcache_append_varlen_ex" and rq is None and q8 is not None and p.rotary_cos is None and p.block_table is None
    assert list(p.kc_stride) == [cap * Hk * D, D, Hk * D] and list(p.vc_stride) == [2 * cap * Hk * D, D, Hk * D] and p.dtype == _lib.TFA_F16
    assert list(q8.k_descale_stride) == [Hk, 1]
    kc, vc = _meta(B, cap, Hk, D, dtype=torch.float16), _meta(B, cap, Hk, D, dtype=torch.float16)
    qkv = _meta(total, H + 2 * Hk, D, dtype=torch.float16)
    cos = _meta(64, 32, dtype=torch.float16)
    ops.kvcache_append_varlen(qkv[:, H:H + Hk], qkv[:, H + Hk:], kc, vc, cu, lens, rotary_cos=cos, rotary_sin=cos, rotary_interleaved=True, q=qkv[:, :H])
    p, q8, rq = _args(stub.calls[1])
    assert stub.calls[1][0] == "tfa_kvcache_append_varlen_ex" and q8 is None
    assert (rq.q, rq.H) == (_ptr(qkv), H) and list(rq.q_stride) == [D, (H + 2 * Hk) * D] and p.k == rq.q + H * D * 2 and p.rotary_interleaved == 1


def test_wrapper_without_the_new_keywords_reaches_the_old_symbol(stub):
    total, Hk, D, B = 6, 2, 64, 2
    k, v, kc, vc = _meta(total, Hk, D), _meta(total, Hk, D), _meta(5, 64, Hk, D), _meta(5, 64, Hk, D)
    cu, lens, bt = _i32(B + 1), _i32(B), _i32(B, 3)
    cos = _meta(32, 16)
    ops.kvcache_append_varlen(k, v, kc, vc, cu, lens, bt)
    ops.kvcache_append_varlen(k, v, kc, vc, cu, lens, bt, rotary_cos=cos, rotary_sin=cos)
    ops.kvcache_append_varlen(k, v, kc, vc, cu, lens, bt, rotary_cos=cos, rotary_sin=cos, q=None, k_descale=None, v_descale=None)
    assert [c[0] for c in stub.calls] == ["tfa_kvcache_append_varlen"] * 3
    assert all(len(c[1]) == 2 for c in stub.calls)                               # (params, stream): the old prototype


def test_wrapper_refuses_by_name_before_any_call(stub):
    f = ops.kvcache_append_varlen
    B, total, H, Hk, D = 2, 6, 8, 2, 64
    k, v, kc, vc = _meta(total, Hk, D), _meta(total, Hk, D), _meta(5, 64, Hk, D), _meta(5, 64, Hk, D)
    k8, v8 = _meta(5, 64, Hk, D, dtype=E4M3), _meta(5, 64, Hk, D, dtype=E4M3)
    cu, lens, bt = _i32(B + 1), _i32(B), _i32(B, 3)
    d = _meta(B, Hk, dtype=torch.float32)
    q, cos = _meta(total, H, D), _meta(32, 16)
    rot = dict(rotary_cos=cos, rotary_sin=cos)
    # the pinned sentence: an fp8 cache without both descales
    for kw in (dict(), dict(k_descale=d), dict(v_descale=d)):
        with pytest.raises(TypeError, match="fp8 caches are not served without k_descale / v_descale"):
            f(k, v, k8, v8, cu, lens, bt, **kw)
    # descales with 16-bit caches
    for kw in (dict(k_descale=d), dict(v_descale=d), dict(k_descale=d, v_descale=d)):
        with pytest.raises(TypeError, match="belong to torch.float8_e4m3fn caches"):
            f(k, v, kc, vc, cu, lens, bt, **kw)
    # other fp8 formats, mixed cache dtypes
    for other in (torch.float8_e5m2, torch.float8_e4m3fnuz):
        c8 = _meta(5, 64, Hk, D, dtype=other)
        with pytest.raises(TypeError, match="float8_e5m2 and float8_e4m3fnuz caches are not supported"):
            f(k, v, c8, c8, cu, lens, bt, k_descale=d, v_descale=d)
        with pytest.raises(TypeError, match="share one dtype"):
            f(k, v, k8, c8, cu, lens, bt, k_descale=d, v_descale=d)
    for pair in ((k8, vc), (kc, v8)):
        with pytest.raises(TypeError, match="share one dtype"):
            f(k, v, *pair, cu, lens, bt, k_descale=d, v_descale=d)
    # a descale of the wrong dtype, shape or device
    for bad in (_meta(B, Hk, dtype=torch.float16), _meta(B, Hk, dtype=torch.float64), 1.0, [[1.0] * Hk] * B):
        with pytest.raises(TypeError, match="k_descale must be a float32 tensor"):
            f(k, v, k8, v8, cu, lens, bt, k_descale=bad, v_descale=d)
    for bad in (_meta(B, Hk + 1, dtype=torch.float32), _meta(B + 1, Hk, dtype=torch.float32), _meta(Hk, dtype=torch.float32), _meta(5, Hk, dtype=torch.float32),
                torch.ones(B, Hk)):
        with pytest.raises(TypeError, match=r"v_descale must have shape \(2, 2\)"):
            f(k, v, k8, v8, cu, lens, bt, k_descale=d, v_descale=bad)
    # an fp8 head dim that is not a multiple of 16; a pool whose strides are not multiples of 16 bytes
    with pytest.raises(ValueError, match="multiple of 16"):
        f(_meta(total, Hk, 40), _meta(total, Hk, 40), _meta(5, 64, Hk, 40, dtype=E4M3), _meta(5, 64, Hk, 40, dtype=E4M3), cu, lens, bt, k_descale=d, v_descale=d)
    with pytest.raises(ValueError, match="16-byte aligned rows"):
        f(k, v, _meta(5, 64, Hk, D + 8, dtype=E4M3)[..., :D], v8, cu, lens, bt, k_descale=d, v_descale=d)
    # q
    with pytest.raises(ValueError, match="needs them"):
        f(k, v, kc, vc, cu, lens, bt, q=q)
    for bad in (1.0, [q]):
        with pytest.raises(TypeError, match="q must be a tensor"):
            f(k, v, kc, vc, cu, lens, bt, q=bad, **rot)
    with pytest.raises(TypeError, match="q must have k's dtype"):
        f(k, v, kc, vc, cu, lens, bt, q=_meta(total, H, D, dtype=torch.float16), **rot)
    for bad in (_meta(1, total, H, D), _meta(total, H * D), _meta(total + 1, H, D), _meta(total - 1, H, D), _meta(total, H, 2 * D), _meta(total, 0, D)):
        with pytest.raises(ValueError, match="q must be 3-D"):
            f(k, v, kc, vc, cu, lens, bt, q=bad, **rot)
    with pytest.raises(ValueError, match="q must be on k's device"):
        f(k, v, kc, vc, cu, lens, bt, q=torch.empty(total, H, D, dtype=torch.bfloat16), **rot)
    for bad in (_meta(total, D, H).transpose(1, 2), _meta(total, H, D + 4)[..., :D], _meta(total, H, 2 * D)[..., ::2]):
        with pytest.raises(ValueError, match="q must have unit stride"):
            f(k, v, kc, vc, cu, lens, bt, q=bad, **rot)
    with pytest.raises(ValueError, match="16-byte aligned address"):
        f(k, v, kc, vc, cu, lens, bt, q=_meta(total * H * D + 4).narrow(0, 4, total * H * D).view(total, H, D), **rot)
    with pytest.raises(RuntimeError, match="not differentiable"):
        f(k, v, kc, vc, cu, lens, bt, q=_meta(total, H, D).requires_grad_(True), **rot)
    with pytest.raises(RuntimeError, match="not differentiable"):
        f(k, v, k8, v8, cu, lens, bt, q=_meta(total, H, D).requires_grad_(True), k_descale=d, v_descale=d, **rot)
    assert stub.calls == []
    f(k, v, k8, v8, cu, lens, bt, q=q, k_descale=d, v_descale=d, **rot)
    assert [c[0] for c in stub.calls] == ["tfa_kvcache_append_varlen_ex"]
