"""CPU tests of the K/V-cache entry points (include/tfa.h: tfa_fwd_kvcache, _workspace, _plan, _suggest_splits, tfa_kvcache_append) and of the Python
wrapper ``flash_attn_with_kvcache``: symbols, plans of contiguous and paged caches, refusal codes, workspace sizes, the split suggestion's bounds, and the
wrapper's host-side behaviour against a counting stand-in for the library.  No GPU: plans never launch, refused calls return before any launch, the
lengths and the block table are never read on the host (a stand-in address serves)."""
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
KVC_SYMBOLS = ("tfa_fwd_kvcache", "tfa_fwd_kvcache_workspace", "tfa_fwd_kvcache_plan", "tfa_fwd_kvcache_suggest_splits", "tfa_kvcache_append")


def params(B=4, H=32, Hk=8, Nq=1, D=128, cap=4096, page=0, num_pages=None, n_new=0, causal=False, dtype=_lib.TFA_BF16, dense_out=True):
    """A tfa_kvcache_params over FlashAttention-2's layouts: q (B, Nq, H, D), caches (B, cap, Hk, D) or paged (num_pages, page, Hk, D) with a
    (B, cap / page) block table, out dense (B, H, Nq, D) — or laid out like q."""
    p = _lib.TfaKvcacheParams()
    p.q = p.out = p.lse = p.k_cache = p.v_cache = p.cache_seqlens = ADDR
    p.B, p.H, p.Hk, p.Nq, p.D, p.capacity = B, H, Hk, Nq, D, cap
    p.q_stride[0], p.q_stride[1], p.q_stride[2] = Nq * H * D, D, H * D
    if dense_out:
        p.o_stride[0], p.o_stride[1], p.o_stride[2] = H * Nq * D, Nq * D, D
    else:
        p.o_stride[0], p.o_stride[1], p.o_stride[2] = Nq * H * D, D, H * D
    rows = page if page else cap
    for name in ("k_stride", "v_stride"):
        arr = getattr(p, name)
        arr[0], arr[1], arr[2] = rows * Hk * D, D, Hk * D
    if page:
        p.block_table = ADDR
        p.page_size = page
        p.num_pages = num_pages if num_pages is not None else B * (cap // page)
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


def plan(p, splits=1):
    g, b, l = C.c_int(), C.c_int(), C.c_int()
    return _lib.lib().tfa_fwd_kvcache_plan(C.byref(p), splits, C.byref(g), C.byref(b), C.byref(l)), g.value, b.value, l.value


def test_symbols_exported_and_version():
    L = _lib.lib()
    for s in KVC_SYMBOLS:
        assert s in _lib.SYMBOLS
        getattr(L, s)
    assert L.tfa_version() == 111


def test_struct_size_matches_the_header():
    """The ctypes mirror and the C struct agree in size (a C program prints sizeof)."""
    src = '#include <stdio.h>\n#include "tfa.h"\nint main(void) { printf("%zu", sizeof(tfa_kvcache_params)); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        assert int(subprocess.check_output([exe]).decode()) == C.sizeof(_lib.TfaKvcacheParams)


@pytest.mark.parametrize("D,lds", [(64, 4 * 64 * 64 * 2), (128, 4 * 64 * 128 * 2), (40, 4 * 64 * 64 * 2), (104, 4 * 64 * 128 * 2)])
@pytest.mark.parametrize("page", [0, 64, 256])
@pytest.mark.parametrize("splits", [1, 2, 8])
def test_plans_of_accepted_geometries(D, lds, page, splits):
    """Contiguous and paged, one chunk and more, GQA, MQA and MHA, decode and several rows: grid = work items x chunks, 256 threads, two K and two V buffers."""
    B, cap = 4, 4096
    for H, Hk, Nq, causal, items in ((32, 8, 1, False, B * 8),        # GQA decode: packed, one item per K/V head
                                     (16, 1, 1, True, B * 1),          # MQA decode: packed (a causal mask hides nothing from one row)
                                     (8, 8, 1, False, B * 8),          # MHA decode
                                     (32, 8, 5, True, B * 32),         # speculative decode: unpacked, one item per query head
                                     (4, 2, 300, True, B * 4 * 2),     # three 128-row blocks, causal pairs: two work items per head
                                     (4, 2, 300, False, B * 4 * 3)):
        for dtype in (_lib.TFA_BF16, _lib.TFA_F16):
            p = params(B=B, H=H, Hk=Hk, Nq=Nq, D=D, cap=cap, page=page, causal=causal, dtype=dtype)
            st, grid, block, l = plan(p, splits)
            assert (st, grid, block, l) == (0, items * splits, 256, lds), (H, Hk, Nq, causal)
            p = params(B=B, H=H, Hk=Hk, Nq=Nq, D=D, cap=cap, page=page, n_new=3, causal=causal, dtype=dtype)
            assert plan(p, splits)[:2] == (0, items * splits)


def test_one_chunk_takes_any_out_strides_more_chunks_a_dense_out():
    p = params(Nq=5, dense_out=False)
    assert plan(p, 1)[0] == 0
    assert plan(p, 2)[0] == CODES["TFA_ERR_STRIDE"]
    assert _lib.lib().tfa_fwd_kvcache_workspace(C.byref(p), 2) == CODES["TFA_ERR_STRIDE"]


def test_chunks_never_outnumber_the_tiles_of_the_capacity():
    L = _lib.lib()
    p = params(cap=192, H=8, Hk=8)
    assert plan(p, 8)[1] == 4 * 8 * 3
    assert L.tfa_fwd_kvcache_workspace(C.byref(p), 8) == 3 * 4 * 8 * 1 * 129
    p = params(cap=64, H=8, Hk=8)
    assert plan(p, 8)[1] == 4 * 8 and L.tfa_fwd_kvcache_workspace(C.byref(p), 8) == 0


@pytest.mark.parametrize("page", [0, 128])
@pytest.mark.parametrize("B,H,Hk,Nq,D", [(4, 32, 8, 1, 128), (3, 8, 8, 1, 64), (2, 16, 1, 1, 104), (2, 8, 2, 17, 40)])
def test_workspace_size_matches_what_the_launch_uses(page, B, H, Hk, Nq, D):
    """One chunk: no workspace.  More: fp32 partial O (D floats) and LSE (1 float) per chunk and output row — the rows keep their count under GQA packing,
    and the grid the plan reports carries exactly that many chunks."""
    L = _lib.lib()
    p = params(B=B, H=H, Hk=Hk, Nq=Nq, D=D, page=page)
    assert L.tfa_fwd_kvcache_workspace(C.byref(p), 1) == 0
    for splits in (2, 5, 16):
        assert L.tfa_fwd_kvcache_workspace(C.byref(p), splits) == splits * B * H * Nq * (D + 1)
        assert plan(p, splits)[1] == plan(p, 1)[1] * splits
    assert L.tfa_fwd_kvcache_workspace(C.byref(p), 0) == CODES["TFA_ERR_SHAPE"]


def test_launch_refuses_a_missing_or_misaligned_workspace_before_any_launch():
    L = _lib.lib()
    p = params()
    assert L.tfa_fwd_kvcache(C.byref(p), 4, None, None) == CODES["TFA_ERR_NULL"]
    assert L.tfa_fwd_kvcache(C.byref(p), 4, ADDR + 4, None) == CODES["TFA_ERR_ALIGN"]


@pytest.mark.parametrize("D", [0, 4, 12, 136, 256])
def test_refusal_head_dim(D):
    assert plan(params(D=D))[0] == CODES["TFA_ERR_HEAD_DIM"]
    assert _lib.lib().tfa_kvcache_append(C.byref(params(D=D, n_new=1)), None) == CODES["TFA_ERR_HEAD_DIM"]


@pytest.mark.parametrize("dtype", [_lib.TFA_F32, 7, -1])
def test_refusal_dtype(dtype):
    assert plan(params(dtype=dtype))[0] == CODES["TFA_ERR_DTYPE"]
    assert _lib.lib().tfa_fwd_kvcache_workspace(C.byref(params(dtype=dtype)), 2) == CODES["TFA_ERR_DTYPE"]


@pytest.mark.parametrize("page", [-64, 1, 32, 96, 100, 65])
def test_refusal_page_size(page):
    p = params(page=64)
    p.page_size = page
    assert plan(p)[0] == CODES["TFA_ERR_SHAPE"]
    p = params(page=64, n_new=1)
    p.page_size = page
    assert _lib.lib().tfa_kvcache_append(C.byref(p), None) == CODES["TFA_ERR_SHAPE"]


def test_refusal_paged_geometry():
    p = params(page=128)
    p.capacity = 4096 + 64                                  # not whole pages
    assert plan(p)[0] == CODES["TFA_ERR_SHAPE"]
    p = params(page=128)
    p.num_pages = 0
    assert plan(p)[0] == CODES["TFA_ERR_SHAPE"]
    p = params(page=128)
    p.block_table_stride = 4096 // 128 - 1                  # rows of the table overlap
    assert plan(p)[0] == CODES["TFA_ERR_STRIDE"]
    p = params(page=128)
    p.block_table = ADDR + 2
    assert plan(p)[0] == CODES["TFA_ERR_ALIGN"]


@pytest.mark.parametrize("field", ["q", "out", "k_cache", "v_cache", "cache_seqlens"])
def test_refusal_null_pointers(field):
    p = params()
    setattr(p, field, None)
    assert plan(p)[0] == CODES["TFA_ERR_NULL"]
    assert _lib.lib().tfa_fwd_kvcache(C.byref(p), 1, None, None) == CODES["TFA_ERR_NULL"]


def test_refusal_null_params_and_half_a_new_pair():
    L = _lib.lib()
    assert L.tfa_fwd_kvcache_plan(None, 1, None, None, None) == CODES["TFA_ERR_NULL"]
    assert L.tfa_fwd_kvcache(None, 1, None, None) == CODES["TFA_ERR_NULL"]
    assert L.tfa_fwd_kvcache_workspace(None, 1) == CODES["TFA_ERR_NULL"]
    assert L.tfa_kvcache_append(None, None) == CODES["TFA_ERR_NULL"]
    assert L.tfa_fwd_kvcache_suggest_splits(None) == 1
    p = params(n_new=1)
    p.v_new = None
    assert plan(p)[0] == CODES["TFA_ERR_NULL"] and L.tfa_kvcache_append(C.byref(p), None) == CODES["TFA_ERR_NULL"]
    assert L.tfa_kvcache_append(C.byref(params()), None) == CODES["TFA_ERR_NULL"]          # the append alone needs k_new / v_new
    p = params(n_new=1)
    p.n_new = 0
    assert plan(p)[0] == CODES["TFA_ERR_SHAPE"]
    p = params()
    p.n_new = 1                                                                           # rows announced, none given
    assert plan(p)[0] == CODES["TFA_ERR_SHAPE"]


@pytest.mark.parametrize("field", ["q", "out", "k_cache", "v_cache", "k_new", "v_new"])
def test_refusal_misaligned_pointers(field):
    p = params(n_new=1)
    setattr(p, field, ADDR + 8)
    assert plan(p)[0] == CODES["TFA_ERR_ALIGN"]


def test_refusal_misaligned_lengths_and_lse():
    p = params()
    p.cache_seqlens = ADDR + 2
    assert plan(p)[0] == CODES["TFA_ERR_ALIGN"]
    p = params()
    p.lse = ADDR + 2
    assert plan(p)[0] == CODES["TFA_ERR_ALIGN"] and plan(p, 4)[0] == CODES["TFA_ERR_ALIGN"]


@pytest.mark.parametrize("kw", [dict(B=0), dict(H=0), dict(Hk=0), dict(Nq=0), dict(cap=0), dict(H=12, Hk=8)])
def test_refusal_shapes(kw):
    assert plan(params(**kw))[0] == CODES["TFA_ERR_SHAPE"]


def test_refusal_splits_scale_reserved():
    assert plan(params(), 0)[0] == CODES["TFA_ERR_SHAPE"] and plan(params(), -3)[0] == CODES["TFA_ERR_SHAPE"]
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        p = params()
        p.softmax_scale = bad
        assert plan(p)[0] == CODES["TFA_ERR_SCALE"]
    p = params()
    p.reserved_ = 1
    assert plan(p)[0] == CODES["TFA_ERR_SHAPE"]


@pytest.mark.parametrize("name", ["k_stride", "v_stride", "q_stride", "knew_stride"])
def test_refusal_strides(name):
    p = params(n_new=2, Nq=5)
    getattr(p, name)[2] = 64                     # rows overlap (D = 128)
    assert plan(p)[0] == CODES["TFA_ERR_STRIDE"]
    p = params(n_new=2, Nq=5)
    getattr(p, name)[0] = -1024
    assert plan(p)[0] == CODES["TFA_ERR_STRIDE"]
    p = params(n_new=2, Nq=5)
    getattr(p, name)[1] = 132                    # a head 264 bytes on: rows no longer 16-byte aligned
    assert plan(p)[0] == CODES["TFA_ERR_STRIDE"]


def test_refusal_slice_beyond_one_descriptor_contiguous_only():
    """A contiguous (b, h) slice of 2 GiB and more is refused; the same rows in pages are fine (a descriptor spans one tile of one page)."""
    cap, Hk, D = 1 << 17, 64, 128                # rows 16 KiB apart x 131072 keys = 2 GiB per slice
    p = params(B=1, H=64, Hk=Hk, D=D, cap=cap)
    assert plan(p)[0] == CODES["TFA_ERR_STRIDE"]
    assert _lib.lib().tfa_kvcache_append(C.byref(params(B=1, H=64, Hk=Hk, D=D, cap=cap, n_new=1)), None) == CODES["TFA_ERR_STRIDE"]
    assert plan(params(B=1, H=64, Hk=Hk, D=D, cap=cap, page=256))[0] == 0
    assert plan(params(B=1, H=64, Hk=Hk, D=D, cap=cap // 2))[0] == 0


def test_suggest_splits_bounds():
    L = _lib.lib()
    sug = lambda **kw: L.tfa_fwd_kvcache_suggest_splits(C.byref(params(**kw)))
    cus = 256                                    # what the library assumes without a device (MI355X)
    assert sug(B=64, H=32, Hk=8, cap=16384) == 1                      # 512 packed work items: the grid fills the chip
    assert sug(B=32, H=8, Hk=8, cap=16384) == 1                       # 256 items on more than half of the CUs
    assert sug(B=1, H=32, Hk=8, cap=2048) == 1                        # too few keys to be worth a merge
    assert sug(B=1, H=32, Hk=8, cap=16384) == min(32, 16384 // 1024, cus // 8) == 16
    assert sug(B=8, H=32, Hk=8, cap=16384) == cus // 64 == 4
    assert sug(B=8, H=32, Hk=8, cap=16384, page=256) == 4             # the layout does not matter
    assert sug(B=1, H=8, Hk=8, cap=1 << 20) == 32                     # never more than 32
    assert sug(B=12, H=64, Hk=8, cap=32768) == 2 * cus // 96 == 5     # between a quarter and a half of the CUs: two workgroups per CU
    assert sug(B=1, H=32, Hk=8, Nq=5, cap=16384, causal=True) == cus // 32 == 8   # unpacked: one item per query head
    assert sug(B=1, H=8, Hk=8, Nq=2048, cap=4096, causal=True) == 1   # causal prefill: the late chunks serve few rows
    for kw in (dict(B=1), dict(B=8), dict(B=64), dict(B=3, cap=100000, page=0)):
        assert 1 <= sug(**kw) <= 32


def test_header_still_compiles_as_plain_c():
    src = '#include "tfa.h"\nint main(void) { tfa_kvcache_params p; (void)p; (void)tfa_fwd_kvcache; (void)tfa_kvcache_append; return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "h.c")
        open(c, "w").write(src)
        subprocess.check_call(["cc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", c, "-o", os.path.join(d, "h.o")])


# ---- Python: flash_attn_with_kvcache against a counting stand-in for the library -----------------------------------------------------------
class _CountingLib:
    """A stand-in for the loaded library object: records every call, answers TFA_OK, a fixed split suggestion and the real workspace formula."""

    def __init__(self, suggest=4):
        self.calls, self.suggest = [], suggest

    def __getattr__(self, name):
        def f(*a):
            self.calls.append((name, a))
            if name == "tfa_fwd_kvcache_suggest_splits":
                return self.suggest
            if name == "tfa_fwd_kvcache_workspace":
                p, s = a[0]._obj, a[1]
                return s * p.B * p.H * p.Nq * (p.D + 1) if s > 1 else 0
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


def test_wrapper_is_exported():
    import tiny_flash_attention_amd as tfa

    assert tfa.flash_attn_with_kvcache is ops.flash_attn_with_kvcache and "flash_attn_with_kvcache" in tfa.__all__


def test_wrapper_contiguous_call_passes_pointers_and_strides(stub):
    B, Nq, H, Hk, D, cap = 3, 1, 16, 4, 64, 1024
    q = _meta(B, Nq, H, D)
    kc, vc = _meta(B, cap, Hk, D), _meta(B, 2 * cap, Hk, D)[:, :cap]          # v: a strided view
    lens = _meta(B, dtype=torch.int32)
    out, lse = ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, num_splits=2, return_softmax_lse=True)
    assert [c[0] for c in stub.calls] == ["tfa_fwd_kvcache_workspace", "tfa_fwd_kvcache"]
    name, (pref, splits, ws, stream) = stub.calls[-1]
    p = pref._obj
    assert splits == 2 and ws is not None
    assert (p.B, p.H, p.Hk, p.Nq, p.D, p.capacity, p.n_new) == (B, H, Hk, Nq, D, cap, 0)
    assert p.block_table is None and p.k_new is None and p.v_new is None
    assert (p.q, p.k_cache, p.v_cache, p.cache_seqlens) == (q.data_ptr(), kc.data_ptr(), vc.data_ptr(), lens.data_ptr())
    assert list(p.q_stride) == [Nq * H * D, D, H * D]
    assert list(p.k_stride) == [cap * Hk * D, D, Hk * D]
    assert list(p.v_stride) == [2 * cap * Hk * D, D, Hk * D]
    assert list(p.o_stride) == [H * Nq * D, Nq * D, D]                        # the dense (B, H, Nq, D) result the merge writes
    assert p.dtype == _lib.TFA_BF16 and p.is_causal == 0 and abs(p.softmax_scale - 0.125) < 1e-7
    assert tuple(out.shape) == (B, Nq, H, D) and tuple(lse.shape) == (B, H, Nq) and lse.dtype == torch.float32
    assert out.stride() == (H * Nq * D, D, Nq * D, 1)                         # a transposed view of it


def test_wrapper_paged_call_passes_table_and_page_geometry(stub):
    B, Nq, H, Hk, D, page, nb, mb = 2, 5, 8, 2, 128, 128, 40, 12
    q = _meta(B, Nq, H, D, dtype=torch.float16)
    kc, vc = _meta(nb, page, Hk, D, dtype=torch.float16), _meta(nb, page, Hk, D, dtype=torch.float16)
    bt = _meta(B, 16, dtype=torch.int32)[:, :mb]                              # rows 16 entries apart
    lens = _meta(B, dtype=torch.int32)
    out = ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, block_table=bt, causal=True, num_splits=1, softmax_scale=0.5)
    assert [c[0] for c in stub.calls] == ["tfa_fwd_kvcache_workspace", "tfa_fwd_kvcache"]
    pref, splits, ws, _ = stub.calls[-1][1]
    p = pref._obj
    assert splits == 1 and ws is None
    assert (p.page_size, p.num_pages, p.capacity, p.block_table_stride) == (page, nb, mb * page, 16)
    assert p.block_table == bt.data_ptr() and p.lse is None
    assert list(p.k_stride) == [page * Hk * D, D, Hk * D] and list(p.v_stride) == [page * Hk * D, D, Hk * D]
    assert p.dtype == _lib.TFA_F16 and p.is_causal == 1 and p.softmax_scale == 0.5
    assert tuple(out.shape) == (B, Nq, H, D)


def test_wrapper_append_is_one_library_call_with_the_new_rows(stub):
    """k / v given: the one tfa_fwd_kvcache call carries them — the library appends first, then attends, on the same stream (include/tfa.h); the wrapper itself
    launches nothing else and does not touch cache_seqlens."""
    B, H, Hk, D, cap, n_new = 2, 8, 8, 64, 512, 3
    q, kc, vc = _meta(B, 1, H, D), _meta(B, cap, Hk, D), _meta(B, cap, Hk, D)
    k, v = _meta(B, n_new, Hk, D), _meta(B, n_new, Hk, D)
    ops.flash_attn_with_kvcache(q, kc, vc, k, v, cache_seqlens=_meta(B, dtype=torch.int32), num_splits=1)
    assert [c[0] for c in stub.calls] == ["tfa_fwd_kvcache_workspace", "tfa_fwd_kvcache"]
    p = stub.calls[-1][1][0]._obj
    assert p.n_new == n_new and p.k_new == k.data_ptr() and p.v_new == v.data_ptr()
    assert list(p.knew_stride) == [n_new * Hk * D, D, Hk * D] and list(p.vnew_stride) == [n_new * Hk * D, D, Hk * D]


def test_wrapper_auto_splits_asks_the_library(stub):
    q, kc = _meta(1, 1, 8, 64), _meta(1, 8192, 8, 64)
    ops.flash_attn_with_kvcache(q, kc, kc)
    assert [c[0] for c in stub.calls] == ["tfa_fwd_kvcache_suggest_splits", "tfa_fwd_kvcache_workspace", "tfa_fwd_kvcache"]
    assert stub.calls[-1][1][1] == 4 and stub.calls[1][1][1] == 4
    stub.calls.clear()
    ops.flash_attn_with_kvcache(q, kc, kc, cache_seqlens=100, num_splits=3)    # a host int is broadcast
    assert [c[0] for c in stub.calls] == ["tfa_fwd_kvcache_workspace", "tfa_fwd_kvcache"] and stub.calls[-1][1][1] == 3


def test_wrapper_refuses_by_name_before_any_call(stub):
    q, kc = _meta(2, 1, 8, 64), _meta(2, 256, 8, 64)
    f = ops.flash_attn_with_kvcache
    t = _meta(4, dtype=torch.float32)
    for kw in (dict(rotary_cos=t), dict(rotary_sin=t), dict(cache_batch_idx=t), dict(cache_leftpad=t), dict(alibi_slopes=t), dict(window_size=(64, 0)),
               dict(softcap=30.0)):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            f(q, kc, kc, **kw)
    q32 = _meta(2, 1, 8, 64, dtype=torch.float32)
    with pytest.raises(ValueError, match="fp32"):
        f(q32, _meta(2, 256, 8, 64, dtype=torch.float32), _meta(2, 256, 8, 64, dtype=torch.float32))
    with pytest.raises(ValueError, match="up to 128"):
        f(_meta(2, 1, 8, 256), _meta(2, 256, 8, 256), _meta(2, 256, 8, 256))
    with pytest.raises(ValueError, match="multiple of 64"):
        f(q, _meta(9, 48, 8, 64), _meta(9, 48, 8, 64), block_table=_meta(2, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="block_table"):
        f(q, _meta(9, 64, 8, 64), _meta(9, 64, 8, 64), block_table=_meta(2, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="together"):
        f(q, kc, kc, k=_meta(2, 1, 8, 64), cache_seqlens=_meta(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="cache_seqlens"):
        f(q, kc, kc, k=_meta(2, 1, 8, 64), v=_meta(2, 1, 8, 64))
    with pytest.raises(ValueError, match="cache_seqlens"):
        f(q, kc, kc, cache_seqlens=_meta(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="num_splits"):
        f(q, kc, kc, num_splits=-1)
    with pytest.raises(ValueError, match="divide"):
        f(q, _meta(2, 256, 3, 64), _meta(2, 256, 3, 64))
    qg = _meta(2, 1, 8, 64).requires_grad_(True)
    with pytest.raises(RuntimeError, match="not differentiable"):
        f(qg, kc, kc)
    assert stub.calls == []
