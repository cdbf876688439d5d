"""CPU tests of the K/V-cache entry points that take the GQA packing from the caller (include/tfa.h: tfa_fwd_kvcache_pack, _pack_workspace, _pack_plan,
_pack_suggest_splits; TFA_PACK_GQA_AUTO / ON / OFF) and of ``flash_attn_with_kvcache(pack_gqa=)``: plan geometry of the packed form, workspace sizes, refusal
codes, the unchanged layout of the existing structs, and the wrapper's choice of entry points against a counting stand-in for the library.  No GPU: plans never
launch, refused calls return before any launch."""
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
AUTO, ON, OFF = 0, 1, 2
PACK_SYMBOLS = ("tfa_fwd_kvcache_pack", "tfa_fwd_kvcache_pack_workspace", "tfa_fwd_kvcache_pack_plan", "tfa_fwd_kvcache_pack_suggest_splits")
BM = 128                # rows of a query block of the KV-cache kernel (four waves of 32 rows: csrc/tfa_fwd_kernel_dma.h)


def params(B=4, H=32, Hk=8, Nq=1, D=128, cap=4096, page=0, num_pages=None, n_new=0, causal=False, dtype=_lib.TFA_BF16, dense_out=True):
    """tests/test_kvcache_abi.py's: a tfa_kvcache_params over FlashAttention-2's layouts — q (B, Nq, H, D), caches (B, cap, Hk, D) or paged, out dense
    (B, H, Nq, D) or laid out like q."""
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


def fp8_params(**kw):
    """The same with an e4m3 cache (strides in bytes = elements) and its second struct."""
    p = params(**kw)
    q8 = _lib.TfaKvcacheFp8()
    q8.format = _lib.TFA_KV_E4M3
    return p, q8


def plan(p, mode, splits=1, q8=None):
    g, b, l = C.c_int(), C.c_int(), C.c_int()
    st = _lib.lib().tfa_fwd_kvcache_pack_plan(C.byref(p), C.byref(q8) if q8 is not None else None, mode, splits, C.byref(g), C.byref(b), C.byref(l))
    return st, g.value, b.value, l.value


def old_plan(p, splits=1):
    g, b, l = C.c_int(), C.c_int(), C.c_int()
    return _lib.lib().tfa_fwd_kvcache_plan(C.byref(p), splits, C.byref(g), C.byref(b), C.byref(l)), g.value, b.value, l.value


def work_items(rows, causal):
    """Work items per head (group) as the kernel walks them: the query blocks, or — causal — pairs of a heavy and a light block (KArgs::nwork)."""
    nmb = (rows + BM - 1) // BM
    return (nmb + 1) // 2 if causal else nmb


def test_symbols_exported_and_version_unchanged():
    L = _lib.lib()
    for s in PACK_SYMBOLS:
        assert s in _lib.SYMBOLS
        getattr(L, s)
    assert L.tfa_version() == 111
    assert (_lib.TFA_PACK_GQA_AUTO, _lib.TFA_PACK_GQA_ON, _lib.TFA_PACK_GQA_OFF) == (AUTO, ON, OFF)


@pytest.mark.parametrize("page", [0, 64, 256])
@pytest.mark.parametrize("splits", [1, 2, 8])
@pytest.mark.parametrize("causal", [False, True])
def test_plan_geometry_of_the_three_modes(page, splits, causal):
    """B3 H8 Hk2 Nq5: 20 packed rows, one query block per K/V head.  ON: a workgroup per (b, hk, chunk); OFF: per (b, h, chunk); AUTO: tfa_fwd_kvcache_plan's."""
    B, H, Hk, Nq, D, cap = 3, 8, 2, 5, 64, 1024
    for dtype in (_lib.TFA_BF16, _lib.TFA_F16):
        p = params(B=B, H=H, Hk=Hk, Nq=Nq, D=D, cap=cap, page=page, causal=causal, dtype=dtype)
        assert plan(p, ON, splits) == (0, B * Hk * 1 * splits, 256, 4 * 64 * 64 * 2)
        assert plan(p, OFF, splits) == (0, B * H * 1 * splits, 256, 4 * 64 * 64 * 2)
        assert plan(p, AUTO, splits) == old_plan(p, splits) == (0, B * H * splits, 256, 4 * 64 * 64 * 2)
        p = params(B=B, H=H, Hk=Hk, Nq=Nq, D=D, cap=cap, page=page, n_new=Nq, causal=causal, dtype=dtype)
        assert plan(p, ON, splits)[:2] == (0, B * Hk * splits)


@pytest.mark.parametrize("splits", [1, 2])
def test_plan_more_than_one_query_block(splits):
    """H16 Hk4 Nq40: 160 packed rows are two query blocks per (b, hk) — two work items, or one causal pair; Nq33: 132 rows, the same count."""
    B, H, Hk, D, cap = 3, 16, 4, 128, 1024
    for Nq in (40, 33):
        rows = Nq * (H // Hk)
        assert (rows + BM - 1) // BM == 2
        for causal in (False, True):
            p = params(B=B, H=H, Hk=Hk, Nq=Nq, D=D, cap=cap, causal=causal)
            assert plan(p, ON, splits) == (0, B * Hk * work_items(rows, causal) * splits, 256, 4 * 64 * 128 * 2)
            assert plan(p, OFF, splits)[:2] == (0, B * H * work_items(Nq, causal) * splits)
    assert work_items(160, True) == 1 and work_items(160, False) == 2
    # five blocks: three causal work items (two pairs and the middle block alone)
    p = params(B=1, H=16, Hk=4, Nq=150, D=64, cap=1024, causal=True)
    assert plan(p, ON)[:2] == (0, 4 * 3) and plan(p, OFF)[:2] == (0, 16 * 1)


def test_plan_one_row_per_sequence_is_todays_packed_call_and_off_unpacks_it():
    p = params(B=4, H=32, Hk=8, Nq=1)
    assert plan(p, ON, 2) == plan(p, AUTO, 2) == old_plan(p, 2) == (0, 4 * 8 * 2, 256, 4 * 64 * 128 * 2)
    assert plan(p, OFF, 2)[:2] == (0, 4 * 32 * 2)
    p = params(B=4, H=16, Hk=1, Nq=1, causal=True)          # MQA
    assert plan(p, ON)[:2] == plan(p, AUTO)[:2] == (0, 4) and plan(p, OFF)[:2] == (0, 4 * 16)


def test_plan_nothing_to_pack_runs_unpacked():
    """H == Hk: ON is the unpacked call.  G = 256 (more than the 128 rows of a query block per position): ON falls back to the unpacked call, as at Nq == 1 —
    packing is an optimisation, never an error (include/tfa.h)."""
    p = params(B=2, H=8, Hk=8, Nq=4, causal=True)
    assert plan(p, ON) == plan(p, OFF) == plan(p, AUTO)
    for Nq in (1, 3):
        p = params(B=2, H=256, Hk=1, Nq=Nq, D=64, cap=1024, causal=True)
        assert plan(p, ON) == plan(p, OFF) == (0, 2 * 256, 256, 4 * 64 * 64 * 2)
    p = params(B=2, H=128, Hk=1, Nq=3, D=64, cap=1024, causal=True)      # G = 128 still packs: 384 rows, three blocks, two causal work items
    assert plan(p, ON)[:2] == (0, 2 * 1 * 2)


def test_plan_packed_takes_any_out_strides_at_one_chunk():
    """out laid out like q — (B, Nq, H, D) — is fine packed at one chunk (rows are written to their own (b, h, t) places); more chunks need the dense out."""
    p = params(B=3, H=8, Hk=2, Nq=5, D=64, cap=1024, dense_out=False, causal=True)
    assert plan(p, ON, 1)[:2] == (0, 3 * 2)
    assert plan(p, ON, 2)[0] == CODES["TFA_ERR_STRIDE"] and plan(p, OFF, 2)[0] == CODES["TFA_ERR_STRIDE"]


def test_plan_fp8_cache():
    p, q8 = fp8_params(B=3, H=8, Hk=2, Nq=4, D=64, cap=1024, causal=True)
    assert plan(p, ON, 2, q8) == (0, 3 * 2 * 2, 256, 4 * 64 * 64 * 2)
    assert plan(p, OFF, 2, q8)[:2] == (0, 3 * 8 * 2)
    g = C.c_int()
    assert _lib.lib().tfa_fwd_kvcache_fp8_plan(C.byref(p), C.byref(q8), 2, C.byref(g), None, None) == 0 and plan(p, AUTO, 2, q8)[1] == g.value == 3 * 8 * 2
    q8.format = 9
    assert plan(p, ON, 2, q8)[0] == CODES["TFA_ERR_DTYPE"]


@pytest.mark.parametrize("page", [0, 128])
@pytest.mark.parametrize("B,H,Hk,Nq,D", [(3, 8, 2, 5, 64), (4, 32, 8, 1, 128), (2, 16, 4, 40, 40), (2, 8, 8, 3, 64)])
def test_workspace_is_the_same_packed_or_not(page, B, H, Hk, Nq, D):
    L = _lib.lib()
    p = params(B=B, H=H, Hk=Hk, Nq=Nq, D=D, cap=1024, page=page)
    for mode in (AUTO, ON, OFF):
        assert L.tfa_fwd_kvcache_pack_workspace(C.byref(p), None, mode, 1) == 0
        for splits in (2, 5):
            assert L.tfa_fwd_kvcache_pack_workspace(C.byref(p), None, mode, splits) == splits * B * H * Nq * (D + 1) == L.tfa_fwd_kvcache_workspace(C.byref(p), splits)
        assert L.tfa_fwd_kvcache_pack_workspace(C.byref(p), None, mode, 64) == 16 * B * H * Nq * (D + 1)      # chunks never outnumber the capacity's tiles


@pytest.mark.parametrize("mode", [3, -1, 4, 1 << 20])
def test_refusal_unknown_pack_mode(mode):
    L = _lib.lib()
    p = params(Nq=4)
    assert plan(p, mode)[0] == CODES["TFA_ERR_SHAPE"]
    assert L.tfa_fwd_kvcache_pack_workspace(C.byref(p), None, mode, 2) == CODES["TFA_ERR_SHAPE"]
    assert L.tfa_fwd_kvcache_pack(C.byref(p), None, mode, 1, None, None) == CODES["TFA_ERR_SHAPE"]
    assert L.tfa_fwd_kvcache_pack_suggest_splits(C.byref(p), mode) == 1


@pytest.mark.parametrize("mode", [AUTO, ON, OFF])
def test_refusals_of_the_plain_plan_arrive_unchanged(mode):
    """A few of tests/test_kvcache_abi.py's table, through the new plan at Nq = 4 (the packed form when ON): the code tfa_fwd_kvcache_plan gives."""
    L = _lib.lib()
    cases = []
    for D in (0, 12, 136):
        cases.append(params(Nq=4, D=D))
    cases.append(params(Nq=4, dtype=_lib.TFA_F32))
    for field in ("q", "out", "k_cache", "cache_seqlens"):
        p = params(Nq=4)
        setattr(p, field, None)
        cases.append(p)
    for field in ("q", "out", "v_cache"):
        p = params(Nq=4)
        setattr(p, field, ADDR + 8)
        cases.append(p)
    for kw in (dict(B=0), dict(Hk=0), dict(Nq=0), dict(cap=0), dict(H=12, Hk=8)):
        cases.append(params(**{**dict(Nq=4), **kw}))
    p = params(Nq=4, page=64)
    p.page_size = 96
    cases.append(p)
    p = params(Nq=4, page=128)
    p.block_table_stride = 4096 // 128 - 1
    cases.append(p)
    for bad in (0.0, float("nan")):
        p = params(Nq=4)
        p.softmax_scale = bad
        cases.append(p)
    for name in ("reserved_", "reserved2_"):                # still "must be 0"
        p = params(Nq=4)
        setattr(p, name, 1)
        cases.append(p)
    for name in ("q_stride", "k_stride"):
        p = params(Nq=4)
        getattr(p, name)[2] = 64
        cases.append(p)
        p = params(Nq=4)
        getattr(p, name)[1] = 132
        cases.append(p)
    p = params(Nq=4)
    p.n_new = 1
    cases.append(p)
    assert len(cases) > 20
    for p in cases:
        want = old_plan(p)[0]
        assert want < 0 and plan(p, mode)[0] == want
    assert plan(params(Nq=4), mode, 0)[0] == CODES["TFA_ERR_SHAPE"]
    assert L.tfa_fwd_kvcache_pack_plan(None, None, mode, 1, None, None, None) == CODES["TFA_ERR_NULL"]
    assert L.tfa_fwd_kvcache_pack(None, None, mode, 1, None, None) == CODES["TFA_ERR_NULL"]
    assert L.tfa_fwd_kvcache_pack_workspace(None, None, mode, 1) == CODES["TFA_ERR_NULL"]
    # a split launch without a workspace, or with a misaligned one: refused before any launch
    p = params(Nq=4)
    assert L.tfa_fwd_kvcache_pack(C.byref(p), None, mode, 4, None, None) == CODES["TFA_ERR_NULL"]
    assert L.tfa_fwd_kvcache_pack(C.byref(p), None, mode, 4, ADDR + 4, None) == CODES["TFA_ERR_ALIGN"]


def test_suggest_splits_counts_the_packed_workgroups():
    L = _lib.lib()
    sug = lambda mode, **kw: L.tfa_fwd_kvcache_pack_suggest_splits(C.byref(params(**kw)), mode)
    cus = 256                                    # what the library assumes without a device (MI355X)
    kw = dict(B=1, H=32, Hk=8, Nq=4, cap=16384, causal=True)
    assert sug(OFF, **kw) == sug(AUTO, **kw) == cus // 32 == 8          # a workgroup per query head
    assert sug(ON, **kw) == min(32, 16384 // 1024, cus // 8) == 16      # ... per K/V head: 16 packed rows, one block
    kw = dict(B=8, H=32, Hk=8, Nq=8, cap=16384, causal=True)
    assert sug(OFF, **kw) == 1 and sug(ON, **kw) == cus // 64 == 4
    kw = dict(B=2, H=32, Hk=8, Nq=40, cap=16384)                        # 160 packed rows: two blocks per (b, hk)
    assert sug(ON, **kw) == cus // (2 * 8 * 2) == 8 and sug(OFF, **kw) == cus // 64 == 4
    kw = dict(B=1, H=32, Hk=8, Nq=1, cap=16384)
    assert sug(ON, **kw) == sug(AUTO, **kw) == 16 and sug(OFF, **kw) == 8
    assert sug(ON, B=1, H=8, Hk=2, Nq=2048, cap=4096, causal=True) == 1  # causal prefill: the late chunks serve few rows, packed or not
    for mode in (AUTO, ON, OFF):
        for kw in (dict(B=1), dict(B=8, Nq=3), dict(B=64, Nq=8), dict(B=3, cap=100000, Nq=2)):
            assert 1 <= sug(mode, **kw) <= 32
            if mode == AUTO:
                assert sug(mode, **kw) == L.tfa_fwd_kvcache_suggest_splits(C.byref(params(**kw)))
    assert L.tfa_fwd_kvcache_pack_suggest_splits(None, ON) == 1


def test_struct_layout_unchanged_and_new_symbols_link():
    """sizeof(tfa_kvcache_params) and sizeof(tfa_kvcache_fp8) are what the ctypes mirrors say (no field was added), and a C program that includes tfa.h links the
    new entry points and gets the codes of a NULL struct and of an unknown mode from them."""
    src = ('#include <stdio.h>\n#include <string.h>\n#include "tfa.h"\n'
           "int main(void) {\n"
           "  tfa_kvcache_params p; int g = 0;\n"
           "  memset(&p, 0, sizeof p);\n"
           "  if (tfa_fwd_kvcache_pack(0, 0, TFA_PACK_GQA_ON, 1, 0, 0) != TFA_ERR_NULL) return 2;\n"
           "  if (tfa_fwd_kvcache_pack_plan(0, 0, TFA_PACK_GQA_OFF, 1, &g, 0, 0) != TFA_ERR_NULL) return 3;\n"
           "  if (tfa_fwd_kvcache_pack_workspace(0, 0, TFA_PACK_GQA_AUTO, 1) != TFA_ERR_NULL) return 4;\n"
           "  if (tfa_fwd_kvcache_pack_suggest_splits(&p, 7) != 1) return 5;\n"
           "  if (TFA_PACK_GQA_AUTO != 0 || TFA_PACK_GQA_ON != 1 || TFA_PACK_GQA_OFF != 2 || tfa_version() != 111) return 6;\n"
           '  printf("%zu %zu", sizeof(tfa_kvcache_params), sizeof(tfa_kvcache_fp8));\n'
           "  return 0;\n}\n")
    libdir = os.path.dirname(_lib.LIB_PATH)
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.check_call(["cc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe,
                               f"-L{libdir}", "-ltfa_hip", f"-Wl,-rpath,{libdir}"])
        sizes = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert sizes == [C.sizeof(_lib.TfaKvcacheParams), C.sizeof(_lib.TfaKvcacheFp8)]
    assert C.sizeof(_lib.TfaKvcacheParams) == 9 * 8 + 10 * 4 + 19 * 8 + 4 * 4      # nine pointers, ten int32, 19 int64, a float and three int32


# ---- Python: flash_attn_with_kvcache(pack_gqa=) against a counting stand-in for the library -------------------------------------------------
class _CountingLib:
    """A stand-in for the loaded library object: records every call, answers TFA_OK, fixed split suggestions and the real workspace formula."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a):
            self.calls.append((name, a))
            if name == "tfa_fwd_kvcache_suggest_splits":
                return 4
            if name == "tfa_fwd_kvcache_pack_suggest_splits":
                return 6
            if name.endswith("_workspace"):
                p, s = a[0]._obj, a[-1]
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


def _tensors(B=2, Nq=4, H=8, Hk=2, D=64, cap=1024, cache_dtype=torch.bfloat16):
    return _meta(B, Nq, H, D), _meta(B, cap, Hk, D, dtype=cache_dtype), _meta(B, cap, Hk, D, dtype=cache_dtype), _meta(B, dtype=torch.int32)


def test_wrapper_none_calls_todays_symbols_only(stub):
    q, kc, vc, lens = _tensors()
    ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, causal=True, pack_gqa=None)
    ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, causal=True, num_splits=2)
    assert [c[0] for c in stub.calls] == ["tfa_fwd_kvcache_suggest_splits", "tfa_fwd_kvcache_workspace", "tfa_fwd_kvcache", "tfa_fwd_kvcache_workspace",
                                          "tfa_fwd_kvcache"]
    stub.calls.clear()
    q, kc, vc, lens = _tensors(cache_dtype=torch.float8_e4m3fn)
    ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, num_splits=1)
    assert [c[0] for c in stub.calls] == ["tfa_fwd_kvcache_fp8_workspace", "tfa_fwd_kvcache_fp8"]


@pytest.mark.parametrize("flag,mode", [(True, ON), (False, OFF)])
def test_wrapper_true_and_false_call_the_new_symbols(stub, flag, mode):
    q, kc, vc, lens = _tensors()
    out, lse = ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, causal=True, pack_gqa=flag, return_softmax_lse=True)
    assert [c[0] for c in stub.calls] == ["tfa_fwd_kvcache_pack_suggest_splits", "tfa_fwd_kvcache_pack_workspace", "tfa_fwd_kvcache_pack"]
    assert stub.calls[0][1][1] == mode
    pref, q8, m, splits = stub.calls[1][1]
    assert q8 is None and m == mode and splits == 6
    pref, q8, m, splits, ws, stream = stub.calls[2][1]
    p = pref._obj
    assert q8 is None and m == mode and splits == 6 and ws is not None
    assert (p.B, p.H, p.Hk, p.Nq, p.D, p.capacity, p.is_causal) == (2, 8, 2, 4, 64, 1024, 1)
    assert list(p.q_stride) == [4 * 8 * 64, 64, 8 * 64] and list(p.o_stride) == [8 * 4 * 64, 4 * 64, 64]      # the tensors are the unpacked call's
    assert tuple(out.shape) == (2, 4, 8, 64) and tuple(lse.shape) == (2, 8, 4)
    stub.calls.clear()
    ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, pack_gqa=flag, num_splits=3)
    assert [c[0] for c in stub.calls] == ["tfa_fwd_kvcache_pack_workspace", "tfa_fwd_kvcache_pack"] and stub.calls[-1][1][2:4] == (mode, 3)


def test_wrapper_fp8_cache_hands_the_descales_to_the_new_symbols(stub):
    q, kc, vc, lens = _tensors(cache_dtype=torch.float8_e4m3fn)
    kd = _meta(2, 2, dtype=torch.float32)
    ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, pack_gqa=True, num_splits=1, k_descale=kd)
    assert [c[0] for c in stub.calls] == ["tfa_fwd_kvcache_pack_workspace", "tfa_fwd_kvcache_pack"]
    q8 = stub.calls[-1][1][1]._obj
    assert q8.format == _lib.TFA_KV_E4M3 and q8.k_descale == kd.data_ptr() and q8.v_descale is None


@pytest.mark.parametrize("bad", [1, 0, "yes", "True", 1.0, (True,)])
def test_wrapper_refuses_anything_but_none_true_false(stub, bad):
    q, kc, vc, lens = _tensors()
    with pytest.raises(TypeError, match="pack_gqa"):
        ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, pack_gqa=bad)
    assert stub.calls == []


def test_wrapper_keyword_only_and_existing_refusals_come_first(stub):
    q, kc, vc, lens = _tensors()
    with pytest.raises(TypeError):
        ops.flash_attn_with_kvcache(q, kc, vc, None, None, lens, None, None, False, 0, False, True)      # no positional slot behind return_softmax_lse
    with pytest.raises(NotImplementedError, match="softcap"):
        ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, softcap=30.0, pack_gqa="yes")
    with pytest.raises(ValueError, match="num_splits"):
        ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, num_splits=-1, pack_gqa="yes")
    assert stub.calls == []
