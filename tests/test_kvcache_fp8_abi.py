"""CPU tests of the fp8 (e4m3) K/V-cache entry points (include/tfa.h: tfa_fwd_kvcache_fp8, _workspace, _plan, tfa_kvcache_append_fp8) and of the
``k_descale`` / ``v_descale`` arguments of ``flash_attn_with_kvcache``: symbols, struct size, plans against the 16-bit plans, refusal codes, and the
wrapper's host-side behaviour against a counting stand-in for the library.  No GPU: plans never launch, refused calls return before any launch."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest
import torch

from tiny_flash_attention_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDR = 0x10000          # a 16-byte aligned stand-in for device pointers (plans never dereference them)
CODES = {"TFA_ERR_NULL": -1, "TFA_ERR_DTYPE": -2, "TFA_ERR_HEAD_DIM": -3, "TFA_ERR_SHAPE": -4, "TFA_ERR_STRIDE": -5, "TFA_ERR_ALIGN": -6}
FP8_SYMBOLS = ("tfa_fwd_kvcache_fp8", "tfa_fwd_kvcache_fp8_workspace", "tfa_fwd_kvcache_fp8_plan", "tfa_kvcache_append_fp8")
E4M3 = torch.float8_e4m3fn


def params(B=4, H=32, Hk=8, Nq=1, D=128, cap=4096, page=0, n_new=0, causal=False, dtype=_lib.TFA_BF16):
    """A tfa_kvcache_params as tests/test_kvcache_abi.py builds it: q (B, Nq, H, D), caches (B, cap, Hk, D) or paged (num_pages, page, Hk, D), out dense
    (B, H, Nq, D).  The cache strides count elements — the same numbers serve a 16-bit cache and (as bytes) an fp8 one."""
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
        p.block_table = ADDR
        p.page_size = page
        p.num_pages = B * (cap // page)
        p.block_table_stride = cap // page
    if n_new:
        p.k_new = p.v_new = ADDR
        p.n_new = n_new
        for name in ("knew_stride", "vnew_stride"):
            arr = getattr(p, name)
            arr[0], arr[1], arr[2] = n_new * Hk * D, D, Hk * D
    p.softmax_scale = 0.125
    p.is_causal = 1 if causal else 0
    p.dtype = dtype
    return p


def fp8(Hk=8, null=False, stride=None):
    s = _lib.TfaKvcacheFp8()
    s.format = _lib.TFA_KV_E4M3
    if not null:
        s.k_descale = s.v_descale = ADDR
        st = stride if stride is not None else (Hk, 1)
        s.k_descale_stride[0], s.k_descale_stride[1] = st
        s.v_descale_stride[0], s.v_descale_stride[1] = st
    return s


def plan8(p, s, splits=1):
    g, b, l = C.c_int(), C.c_int(), C.c_int()
    return _lib.lib().tfa_fwd_kvcache_fp8_plan(C.byref(p), C.byref(s), splits, C.byref(g), C.byref(b), C.byref(l)), g.value, b.value, l.value


def plan16(p, splits=1):
    g, b, l = C.c_int(), C.c_int(), C.c_int()
    return _lib.lib().tfa_fwd_kvcache_plan(C.byref(p), splits, C.byref(g), C.byref(b), C.byref(l)), g.value, b.value, l.value


def test_symbols_exported_declared_and_listed():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "tfa.h")).read()
    for s in FP8_SYMBOLS:
        assert s in _lib.SYMBOLS
        getattr(L, s)
        assert re.search(r"\b(int|long long)\s+" + s + r"\(const tfa_kvcache_params\*[^;]*const tfa_kvcache_fp8\*", hdr), s
    assert re.search(r"#define\s+TFA_KV_E4M3\s+1\b", hdr) and _lib.TFA_KV_E4M3 == 1
    assert L.tfa_version() == 111                        # the layout of tfa_kvcache_params did not move: the version stays


def test_struct_sizes_match_the_header():
    """The ctypes mirrors and the C structs agree in size and in the offsets of the second struct (a C program prints them)."""
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "tfa.h"\nint main(void) { printf("%zu %zu %zu %zu %zu", sizeof(tfa_kvcache_params), '
           'sizeof(tfa_kvcache_fp8), offsetof(tfa_kvcache_fp8, k_descale_stride), offsetof(tfa_kvcache_fp8, v_descale_stride), offsetof(tfa_kvcache_fp8, format)); '
           '(void)tfa_fwd_kvcache_fp8; (void)tfa_fwd_kvcache_fp8_workspace; (void)tfa_fwd_kvcache_fp8_plan; (void)tfa_kvcache_append_fp8; return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.check_call(["cc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    S = _lib.TfaKvcacheFp8
    assert got == [C.sizeof(_lib.TfaKvcacheParams), C.sizeof(S), S.k_descale_stride.offset, S.v_descale_stride.offset, S.format.offset]
    assert C.sizeof(S) == 56


@pytest.mark.parametrize("D,lds", [(64, 4 * 64 * 64 * 2), (128, 4 * 64 * 128 * 2), (48, 4 * 64 * 64 * 2), (112, 4 * 64 * 128 * 2)])
@pytest.mark.parametrize("page", [0, 64, 256])
@pytest.mark.parametrize("splits", [1, 2, 8])
def test_plans_equal_the_16_bit_plans(D, lds, page, splits):
    """Contiguous and paged, one chunk and more, GQA packed, MQA, MHA, speculative and several blocks: the grid of the 16-bit plan for the same geometry, 256
    threads, and the LDS size the header documents — 4 * 64 * W * 2 bytes: the tiles lie DECODED in LDS."""
    B, cap = 4, 4096
    for H, Hk, Nq, causal, items in ((32, 8, 1, False, B * 8), (16, 1, 1, True, B * 1), (8, 8, 1, False, B * 8), (32, 8, 5, True, B * 32),
                                     (4, 2, 300, True, B * 4 * 2), (4, 2, 300, False, B * 4 * 3)):
        for dtype in (_lib.TFA_BF16, _lib.TFA_F16):
            for n_new in (0, 3):
                p = params(B=B, H=H, Hk=Hk, Nq=Nq, D=D, cap=cap, page=page, n_new=n_new, causal=causal, dtype=dtype)
                got = plan8(p, fp8(Hk), splits)
                assert got == (0, items * splits, 256, lds), (H, Hk, Nq, causal, got)
                assert got == plan16(p, splits)
                assert plan8(p, fp8(null=True), splits) == got                       # NULL descales: 1.0
                assert plan8(p, fp8(stride=(0, 0)), splits) == got                   # a broadcast per-tensor scale


@pytest.mark.parametrize("B,H,Hk,Nq,D", [(4, 32, 8, 1, 128), (3, 8, 8, 1, 64), (2, 16, 1, 1, 112), (2, 8, 2, 17, 48)])
def test_workspace_size_is_the_16_bit_one(B, H, Hk, Nq, D):
    L = _lib.lib()
    p, s = params(B=B, H=H, Hk=Hk, Nq=Nq, D=D), fp8(Hk)
    assert L.tfa_fwd_kvcache_fp8_workspace(C.byref(p), C.byref(s), 1) == 0
    for splits in (2, 5, 16):
        assert L.tfa_fwd_kvcache_fp8_workspace(C.byref(p), C.byref(s), splits) == splits * B * H * Nq * (D + 1) == L.tfa_fwd_kvcache_workspace(C.byref(p), splits)
    assert L.tfa_fwd_kvcache_fp8_workspace(C.byref(p), C.byref(s), 0) == CODES["TFA_ERR_SHAPE"]


def test_suggest_splits_serves_fp8_geometry():
    L = _lib.lib()
    assert L.tfa_fwd_kvcache_suggest_splits(C.byref(params(B=8, cap=16384))) == 4
    assert L.tfa_fwd_kvcache_suggest_splits(C.byref(params(B=64, cap=16384))) == 1


def test_refusal_null_second_struct():
    L = _lib.lib()
    p = params(n_new=1)
    assert L.tfa_fwd_kvcache_fp8_plan(C.byref(p), None, 1, None, None, None) == CODES["TFA_ERR_NULL"]
    assert L.tfa_fwd_kvcache_fp8(C.byref(p), None, 1, None, None) == CODES["TFA_ERR_NULL"]
    assert L.tfa_fwd_kvcache_fp8_workspace(C.byref(p), None, 1) == CODES["TFA_ERR_NULL"]
    assert L.tfa_kvcache_append_fp8(C.byref(p), None, None) == CODES["TFA_ERR_NULL"]
    s = fp8()
    assert L.tfa_fwd_kvcache_fp8_plan(None, C.byref(s), 1, None, None, None) == CODES["TFA_ERR_NULL"]
    assert L.tfa_kvcache_append_fp8(C.byref(params()), C.byref(s), None) == CODES["TFA_ERR_NULL"]     # the append alone needs k_new / v_new


@pytest.mark.parametrize("fmt", [0, 2, -1, 7])
def test_refusal_format(fmt):
    s = fp8()
    s.format = fmt
    assert plan8(params(), s)[0] == CODES["TFA_ERR_DTYPE"]
    assert _lib.lib().tfa_kvcache_append_fp8(C.byref(params(n_new=1)), C.byref(s), None) == CODES["TFA_ERR_DTYPE"]


def test_refusal_reserved():
    s = fp8()
    s.reserved_ = 1
    assert plan8(params(), s)[0] == CODES["TFA_ERR_SHAPE"]


@pytest.mark.parametrize("D", [0, 8, 24, 40, 104, 120, 136, 256])
def test_refusal_head_dim(D):
    assert plan8(params(D=D), fp8())[0] == CODES["TFA_ERR_HEAD_DIM"]
    assert _lib.lib().tfa_kvcache_append_fp8(C.byref(params(D=D, n_new=1)), C.byref(fp8()), None) == CODES["TFA_ERR_HEAD_DIM"]


@pytest.mark.parametrize("dtype", [_lib.TFA_F32, 7, -1])
def test_refusal_q_dtype(dtype):
    assert plan8(params(dtype=dtype), fp8())[0] == CODES["TFA_ERR_DTYPE"]


@pytest.mark.parametrize("name", ["k_stride", "v_stride"])
def test_refusal_cache_strides_count_bytes(name):
    """A head 72 elements on: 144 bytes of a 16-bit cache (16-byte aligned, accepted there), 72 bytes of an fp8 cache (refused)."""
    p = params(D=64)
    getattr(p, name)[1] = 72
    assert plan16(p)[0] == 0
    assert plan8(p, fp8())[0] == CODES["TFA_ERR_STRIDE"]
    p = params(D=64, n_new=1)
    getattr(p, name)[2] = 8 * 64 + 8
    assert plan8(p, fp8())[0] == CODES["TFA_ERR_STRIDE"]
    assert _lib.lib().tfa_kvcache_append_fp8(C.byref(p), C.byref(fp8()), None) == CODES["TFA_ERR_STRIDE"]
    p = params(D=64)
    getattr(p, name)[2] = 32                                 # rows overlap
    assert plan8(p, fp8())[0] == CODES["TFA_ERR_STRIDE"]
    p = params(D=64, n_new=2)
    p.knew_stride[1] = 68                                    # the new rows are 16-bit: 136 bytes, not 16-byte aligned
    assert plan8(p, fp8())[0] == CODES["TFA_ERR_STRIDE"]


@pytest.mark.parametrize("which", ["k_descale_stride", "v_descale_stride"])
@pytest.mark.parametrize("i", [0, 1])
def test_refusal_negative_descale_stride(which, i):
    s = fp8()
    getattr(s, which)[i] = -1
    assert plan8(params(), s)[0] == CODES["TFA_ERR_STRIDE"]


@pytest.mark.parametrize("which", ["k_descale", "v_descale"])
def test_refusal_misaligned_descale(which):
    s = fp8()
    setattr(s, which, ADDR + 2)
    assert plan8(params(), s)[0] == CODES["TFA_ERR_ALIGN"]
    s = fp8()
    setattr(s, which, ADDR + 4)                              # 4-byte alignment is all a float needs
    assert plan8(params(), s)[0] == 0
    s = fp8()
    setattr(s, which, None)                                  # one descale given, the other 1.0
    assert plan8(params(), s)[0] == 0


def test_launch_refuses_a_missing_or_misaligned_workspace_before_any_launch():
    L = _lib.lib()
    p, s = params(), fp8()
    assert L.tfa_fwd_kvcache_fp8(C.byref(p), C.byref(s), 4, None, None) == CODES["TFA_ERR_NULL"]
    assert L.tfa_fwd_kvcache_fp8(C.byref(p), C.byref(s), 4, ADDR + 4, None) == CODES["TFA_ERR_ALIGN"]


# ---- Python: flash_attn_with_kvcache against a counting stand-in for the library -----------------------------------------------------------
class _CountingLib:
    """A stand-in for the loaded library object: records every call, answers TFA_OK, a fixed split suggestion and the workspace formula."""

    def __init__(self, suggest=4):
        self.calls, self.suggest = [], suggest

    def __getattr__(self, name):
        def f(*a):
            self.calls.append((name, a))
            if name == "tfa_fwd_kvcache_suggest_splits":
                return self.suggest
            if name in ("tfa_fwd_kvcache_workspace", "tfa_fwd_kvcache_fp8_workspace"):
                p, s = a[0]._obj, a[-1]
                return s * p.B * p.H * p.Nq * (p.D + 1) if s > 1 else 0
            return 0
        return f


class _FakeCuda:
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


def test_signature_ends_in_the_keyword_only_descales():
    import inspect

    ps = list(inspect.signature(ops.flash_attn_with_kvcache).parameters.values())
    assert [x.name for x in ps[-2:]] == ["k_descale", "v_descale"]
    assert all(x.kind is inspect.Parameter.KEYWORD_ONLY and x.default is None for x in ps[-2:])


def test_wrapper_fp8_contiguous_call(stub):
    B, Nq, H, Hk, D, cap = 3, 1, 16, 4, 64, 1024
    q = _meta(B, Nq, H, D)
    kc, vc = _meta(B, cap, Hk, D, dtype=E4M3), _meta(B, 2 * cap, Hk, D, dtype=E4M3)[:, :cap]
    lens = _meta(B, dtype=torch.int32)
    kd = _meta(B, Hk, dtype=torch.float32)
    vd = _meta(1, 1, dtype=torch.float32).expand(B, Hk)                           # a per-tensor scale, broadcast
    out, lse = ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, num_splits=2, return_softmax_lse=True, k_descale=kd, v_descale=vd)
    assert [c[0] for c in stub.calls] == ["tfa_fwd_kvcache_fp8_workspace", "tfa_fwd_kvcache_fp8"]
    name, (pref, sref, splits, ws, stream) = stub.calls[-1]
    p, s = pref._obj, sref._obj
    assert stub.calls[0][1][1]._obj is s and stub.calls[0][1][2] == 2
    assert splits == 2 and ws is not None
    assert (p.B, p.H, p.Hk, p.Nq, p.D, p.capacity, p.n_new) == (B, H, Hk, Nq, D, cap, 0)
    assert (p.q, p.k_cache, p.v_cache, p.cache_seqlens) == (q.data_ptr(), kc.data_ptr(), vc.data_ptr(), lens.data_ptr())
    assert list(p.k_stride) == [cap * Hk * D, D, Hk * D] and list(p.v_stride) == [2 * cap * Hk * D, D, Hk * D]       # elements = bytes
    assert p.dtype == _lib.TFA_BF16                                                # q's dtype, not the cache's
    assert (s.format, s.reserved_) == (_lib.TFA_KV_E4M3, 0)
    assert (s.k_descale, s.v_descale) == (kd.data_ptr(), vd.data_ptr())
    assert list(s.k_descale_stride) == [Hk, 1] and list(s.v_descale_stride) == [0, 0]
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (B, Nq, H, D) and tuple(lse.shape) == (B, H, Nq)


def test_wrapper_fp8_paged_append_and_null_descales(stub):
    B, Nq, H, Hk, D, page, nb, mb, n_new = 2, 5, 8, 2, 128, 128, 40, 12, 5
    q = _meta(B, Nq, H, D, dtype=torch.float16)
    kc, vc = _meta(nb, page, Hk, D, dtype=E4M3), _meta(nb, page, Hk, D, dtype=E4M3)
    k, v = _meta(B, n_new, Hk, D, dtype=torch.float16), _meta(B, n_new, Hk, D, dtype=torch.float16)
    bt = _meta(B, 16, dtype=torch.int32)[:, :mb]
    kd = _meta(Hk, B, dtype=torch.float32).t()                                     # (B, Hk) by strides (1, B)
    ops.flash_attn_with_kvcache(q, kc, vc, k, v, cache_seqlens=_meta(B, dtype=torch.int32), block_table=bt, causal=True, k_descale=kd)
    assert [c[0] for c in stub.calls] == ["tfa_fwd_kvcache_suggest_splits", "tfa_fwd_kvcache_fp8_workspace", "tfa_fwd_kvcache_fp8"]
    pref, sref, splits, ws, _ = stub.calls[-1][1]
    p, s = pref._obj, sref._obj
    assert splits == 4
    assert (p.page_size, p.num_pages, p.capacity, p.block_table_stride) == (page, nb, mb * page, 16)
    assert p.n_new == n_new and p.k_new == k.data_ptr() and p.v_new == v.data_ptr() and p.dtype == _lib.TFA_F16
    assert s.k_descale == kd.data_ptr() and list(s.k_descale_stride) == [1, B]
    assert s.v_descale is None and list(s.v_descale_stride) == [0, 0]              # None: 1.0


def test_wrapper_16_bit_cache_takes_the_entry_points_it_took(stub):
    q, kc = _meta(1, 1, 8, 64), _meta(1, 8192, 8, 64)
    ops.flash_attn_with_kvcache(q, kc, kc)
    assert [c[0] for c in stub.calls] == ["tfa_fwd_kvcache_suggest_splits", "tfa_fwd_kvcache_workspace", "tfa_fwd_kvcache"]
    assert len(stub.calls[-1][1]) == 4                                             # (params, splits, workspace, stream): no second struct
    stub.calls.clear()
    ops.flash_attn_with_kvcache(q, kc, kc, k=_meta(1, 2, 8, 64), v=_meta(1, 2, 8, 64), cache_seqlens=100, num_splits=3)
    assert [c[0] for c in stub.calls] == ["tfa_fwd_kvcache_workspace", "tfa_fwd_kvcache"]


def test_wrapper_fp8_refusals_before_any_call(stub):
    f = ops.flash_attn_with_kvcache
    B, H, Hk, D, cap = 2, 8, 4, 64, 256
    q = _meta(B, 1, H, D)
    k8, k16 = _meta(B, cap, Hk, D, dtype=E4M3), _meta(B, cap, Hk, D)
    d = _meta(B, Hk, dtype=torch.float32)
    lens = _meta(B, dtype=torch.int32)
    for bad in (torch.float8_e5m2, torch.float8_e4m3fnuz, torch.float8_e5m2fnuz, torch.float32, torch.int8, torch.uint8):
        c = _meta(B, cap, Hk, D, dtype=bad)
        with pytest.raises(TypeError, match="dtype"):
            f(q, c, c)
    for kc, vc in ((k8, k16), (k16, k8), (k8, _meta(B, cap, Hk, D, dtype=torch.float8_e5m2)), (k8, _meta(B, cap, Hk, D, dtype=torch.float16))):
        with pytest.raises(TypeError, match="dtype"):                              # mixed cache dtypes
            f(q, kc, vc)
    with pytest.raises(TypeError):                                                 # an fp8 q
        f(_meta(B, 1, H, D, dtype=E4M3), k8, k8)
    for kn, vn in ((_meta(B, 1, Hk, D, dtype=E4M3), _meta(B, 1, Hk, D)), (_meta(B, 1, Hk, D), _meta(B, 1, Hk, D, dtype=E4M3)),
                   (_meta(B, 1, Hk, D, dtype=E4M3), _meta(B, 1, Hk, D, dtype=E4M3))):
        with pytest.raises((TypeError, ValueError), match="dtype"):               # fp8 new rows
            f(q, k8, k8, k=kn, v=vn, cache_seqlens=lens)
    for kw in (dict(k_descale=d), dict(v_descale=d), dict(k_descale=d, v_descale=d)):
        with pytest.raises(ValueError, match="descale"):                           # descales with a 16-bit cache
            f(q, k16, k16, **kw)
    for name in ("k_descale", "v_descale"):
        for bad in (_meta(B, Hk, dtype=torch.float16), _meta(B, Hk, dtype=torch.float64), 0.5, [[1.0] * Hk] * B):
            with pytest.raises(TypeError, match=name):
                f(q, k8, k8, **{name: bad})
        for bad in (_meta(Hk, dtype=torch.float32), _meta(B, Hk + 1, dtype=torch.float32), _meta(B, Hk, 1, dtype=torch.float32), _meta(Hk, B, dtype=torch.float32),
                    _meta(1, dtype=torch.float32), torch.ones(B, Hk, dtype=torch.float32)):                      # wrong shape; the last: wrong device (cpu)
            with pytest.raises(ValueError, match=name):
                f(q, k8, k8, **{name: bad})
    for Dbad in (8, 24, 40, 72, 120):
        c = _meta(B, cap, Hk, Dbad, dtype=E4M3)
        with pytest.raises(ValueError, match="multiple of 16"):
            f(_meta(B, 1, H, Dbad), c, c)
    # what the K/V-cache path refuses today stays refused with an fp8 cache
    with pytest.raises(NotImplementedError, match="softcap"):
        f(q, k8, k8, softcap=30.0)
    with pytest.raises(ValueError, match="up to 128"):
        f(_meta(B, 1, H, 256), _meta(B, cap, Hk, 256, dtype=E4M3), _meta(B, cap, Hk, 256, dtype=E4M3))
    assert stub.calls == []
