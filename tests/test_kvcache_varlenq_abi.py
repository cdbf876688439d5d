"""CPU tests of the K/V-cache entry points for packed ragged query rows (include/tfa.h: tfa_fwd_kvcache_varlen, _workspace, _plan, _suggest_splits; struct
tfa_kvcache_varlen_q) and of ``flash_attn_with_kvcache(cu_seqlens_q=, max_seqlen_q=)``: the struct's layout against the header, plan geometry of the packed and
unpacked varlen-q forms, workspace sizes, every refusal code, the split suggestion on hand-computed cases, unchanged answers of the existing plans, and the
wrapper's calls and refusals against a counting stand-in for the library.  No GPU: plans never launch, refused calls return before any launch."""
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
VQ_SYMBOLS = ("tfa_fwd_kvcache_varlen", "tfa_fwd_kvcache_varlen_workspace", "tfa_fwd_kvcache_varlen_plan", "tfa_fwd_kvcache_varlen_suggest_splits")
BM = 128                # rows of a query block of the KV-cache kernel


def params(B=4, H=32, Hk=8, D=128, cap=4096, total_q=64, page=0, num_pages=None, causal=False, dtype=_lib.TFA_BF16, dense_out=True):
    """A tfa_kvcache_params of the varlen-q call: q (total_q, H, D), out dense (H, total_q, D) or laid out like q, strides {ignored, head, row}; Nq not looked at."""
    p = _lib.TfaKvcacheParams()
    p.q = p.out = p.lse = p.k_cache = p.v_cache = p.cache_seqlens = ADDR
    p.B, p.H, p.Hk, p.Nq, p.D, p.capacity = B, H, Hk, 0, D, cap
    p.q_stride[0], p.q_stride[1], p.q_stride[2] = 0, D, H * D
    if dense_out:
        p.o_stride[0], p.o_stride[1], p.o_stride[2] = 0, total_q * D, D
    else:
        p.o_stride[0], p.o_stride[1], p.o_stride[2] = 0, D, H * D
    rows = page if page else cap
    for name in ("k_stride", "v_stride"):
        arr = getattr(p, name)
        arr[0], arr[1], arr[2] = rows * Hk * D, D, Hk * D
    if page:
        p.block_table = ADDR
        p.page_size = page
        p.num_pages = num_pages if num_pages is not None else B * (cap // page)
        p.block_table_stride = cap // page
    p.softmax_scale = 0.125
    p.is_causal = 1 if causal else 0
    p.dtype = dtype
    return p


def varlen(max_q=16, total_q=64):
    v = _lib.TfaKvcacheVarlenQ()
    v.cu_seqlens_q, v.max_seqlen_q, v.total_q = ADDR, max_q, total_q
    return v


def plan(p, vq, mode=AUTO, splits=1, q8=None):
    g, b, l = C.c_int(), C.c_int(), C.c_int()
    st = _lib.lib().tfa_fwd_kvcache_varlen_plan(C.byref(p) if p is not None else None, C.byref(vq) if vq is not None else None,
                                                C.byref(q8) if q8 is not None else None, mode, splits, C.byref(g), C.byref(b), C.byref(l))
    return st, g.value, b.value, l.value


def work_items(rows, causal):
    nmb = (rows + BM - 1) // BM
    return (nmb + 1) // 2 if causal else nmb


def test_symbols_exported_and_version():
    L = _lib.lib()
    for s in VQ_SYMBOLS:
        assert s in _lib.SYMBOLS
        getattr(L, s)
    assert L.tfa_version() == 111


def test_struct_layout_against_the_header_and_symbols_link():
    """sizeof / offsetof of tfa_kvcache_varlen_q as a C program that includes tfa.h sees them; the existing structs keep their sizes; the new entry points link and
    refuse a NULL struct."""
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include <string.h>\n#include "tfa.h"\n'
           "int main(void) {\n"
           "  tfa_kvcache_params p; tfa_kvcache_varlen_q v; int g = 0;\n"
           "  memset(&p, 0, sizeof p); memset(&v, 0, sizeof v);\n"
           "  if (tfa_fwd_kvcache_varlen(0, 0, 0, TFA_PACK_GQA_AUTO, 1, 0, 0) != TFA_ERR_NULL) return 2;\n"
           "  if (tfa_fwd_kvcache_varlen_plan(&p, 0, 0, TFA_PACK_GQA_OFF, 1, &g, 0, 0) != TFA_ERR_NULL) return 3;\n"
           "  if (tfa_fwd_kvcache_varlen_workspace(0, &v, 0, TFA_PACK_GQA_AUTO, 1) != TFA_ERR_NULL) return 4;\n"
           "  if (tfa_fwd_kvcache_varlen_suggest_splits(&p, &v, 7) != 1) return 5;\n"
           "  if (tfa_version() != 111) return 6;\n"
           '  printf("%zu %zu %zu %zu %zu %zu %zu", sizeof(tfa_kvcache_varlen_q), offsetof(tfa_kvcache_varlen_q, cu_seqlens_q), offsetof(tfa_kvcache_varlen_q, max_seqlen_q),\n'
           "         offsetof(tfa_kvcache_varlen_q, total_q), offsetof(tfa_kvcache_varlen_q, reserved_), sizeof(tfa_kvcache_params), sizeof(tfa_kvcache_fp8));\n"
           "  return 0;\n}\n")
    libdir = os.path.dirname(_lib.LIB_PATH)
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.check_call(["cc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe,
                               f"-L{libdir}", "-ltfa_hip", f"-Wl,-rpath,{libdir}"])
        got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    V = _lib.TfaKvcacheVarlenQ
    assert got == [C.sizeof(V), V.cu_seqlens_q.offset, V.max_seqlen_q.offset, V.total_q.offset, V.reserved_.offset, C.sizeof(_lib.TfaKvcacheParams),
                   C.sizeof(_lib.TfaKvcacheFp8)]
    assert got[:5] == [24, 0, 8, 12, 16]
    assert C.sizeof(_lib.TfaKvcacheParams) == 9 * 8 + 10 * 4 + 19 * 8 + 4 * 4      # no field was added


@pytest.mark.parametrize("page", [0, 64, 256])
@pytest.mark.parametrize("splits", [1, 2, 8])
@pytest.mark.parametrize("causal", [False, True])
def test_plan_geometry_packed_and_unpacked(page, splits, causal):
    """B3 H8 Hk2, max_seqlen_q 5: 20 packed rows, one query block per (sequence, K/V head).  AUTO = ON: a workgroup per (b, hk, chunk); OFF: per (b, h, chunk)."""
    B, H, Hk, D, cap = 3, 8, 2, 64, 1024
    for dtype in (_lib.TFA_BF16, _lib.TFA_F16):
        p, vq = params(B=B, H=H, Hk=Hk, D=D, cap=cap, total_q=9, page=page, causal=causal, dtype=dtype), varlen(5, 9)
        assert plan(p, vq, ON, splits) == plan(p, vq, AUTO, splits) == (0, B * Hk * 1 * splits, 256, 4 * 64 * 64 * 2)
        assert plan(p, vq, OFF, splits) == (0, B * H * 1 * splits, 256, 4 * 64 * 64 * 2)


@pytest.mark.parametrize("splits", [1, 2])
def test_plan_more_than_one_query_block_is_sized_by_max_seqlen_q(splits):
    """H16 Hk4, max_seqlen_q 40: 160 packed rows are two query blocks per (b, hk) — two work items, or one causal pair; 33: 132 rows, the same count.  total_q does
    not size the grid: max_seqlen_q does, even above total_q."""
    B, H, Hk, D, cap = 3, 16, 4, 128, 1024
    for mq in (40, 33):
        rows = mq * (H // Hk)
        for causal in (False, True):
            for tq in (50, 20):
                p, vq = params(B=B, H=H, Hk=Hk, D=D, cap=cap, total_q=tq, causal=causal), varlen(mq, tq)
                assert plan(p, vq, ON, splits) == (0, B * Hk * work_items(rows, causal) * splits, 256, 4 * 64 * 128 * 2)
                assert plan(p, vq, OFF, splits)[:2] == (0, B * H * work_items(mq, causal) * splits)
    p, vq = params(B=1, H=16, Hk=4, D=64, cap=1024, total_q=150, causal=True), varlen(150, 150)      # five blocks: three causal work items
    assert plan(p, vq, ON)[:2] == (0, 4 * 3) and plan(p, vq, OFF)[:2] == (0, 16 * 1)
    p, vq = params(B=2, H=8, Hk=2, D=64, cap=1024, total_q=4096), varlen(2048, 4096)                   # a long chunk: 64 blocks packed, 16 unpacked
    assert plan(p, vq, ON)[:2] == (0, 2 * 2 * 64) and plan(p, vq, OFF)[:2] == (0, 2 * 8 * 16)


def test_plan_group_sizes_that_do_not_pack_run_unpacked():
    """H == Hk (MHA: served by the unpacked instantiations) and G = 256: ON is OFF's launch.  G = 128 still packs."""
    p, vq = params(B=2, H=8, Hk=8, total_q=8, causal=True), varlen(4, 8)
    assert plan(p, vq, ON) == plan(p, vq, OFF) == plan(p, vq, AUTO) == (0, 2 * 8, 256, 4 * 64 * 128 * 2)
    p, vq = params(B=2, H=256, Hk=1, D=64, cap=1024, total_q=6, causal=True), varlen(3, 6)
    assert plan(p, vq, ON) == plan(p, vq, OFF) == (0, 2 * 256, 256, 4 * 64 * 64 * 2)
    p, vq = params(B=2, H=128, Hk=1, D=64, cap=1024, total_q=6, causal=True), varlen(3, 6)       # 384 rows, three blocks, two causal work items
    assert plan(p, vq, ON)[:2] == (0, 2 * 1 * 2)
    p, vq = params(B=5, H=16, Hk=1, total_q=5), varlen(1, 5)                                     # MQA decode
    assert plan(p, vq, ON)[:2] == (0, 5) and plan(p, vq, OFF)[:2] == (0, 5 * 16)


def test_plan_out_strides():
    """One chunk takes any out strides (rows are written to their own (h, q0_b + t) places); more chunks need the dense (H, total_q, D)."""
    p, vq = params(B=3, H=8, Hk=2, D=64, cap=1024, total_q=9, dense_out=False, causal=True), varlen(5, 9)
    assert plan(p, vq, ON, 1)[:2] == (0, 3 * 2) and plan(p, vq, OFF, 1)[:2] == (0, 3 * 8)
    assert plan(p, vq, ON, 2)[0] == CODES["TFA_ERR_STRIDE"] and plan(p, vq, OFF, 2)[0] == CODES["TFA_ERR_STRIDE"]
    p = params(B=3, H=8, Hk=2, D=64, cap=1024, total_q=9)
    p.o_stride[1] = 10 * 64                                  # a head stride that is not total_q * D
    assert plan(p, vq, ON, 1)[0] == 0 and plan(p, vq, ON, 2)[0] == CODES["TFA_ERR_STRIDE"]


def test_plan_fp8_cache():
    p, vq = params(B=3, H=8, Hk=2, D=64, cap=1024, total_q=9, causal=True), varlen(4, 9)
    q8 = _lib.TfaKvcacheFp8()
    q8.format = _lib.TFA_KV_E4M3
    assert plan(p, vq, ON, 2, q8) == (0, 3 * 2 * 2, 256, 4 * 64 * 64 * 2)
    assert plan(p, vq, OFF, 2, q8)[:2] == (0, 3 * 8 * 2)
    q8.format = 9
    assert plan(p, vq, ON, 2, q8)[0] == CODES["TFA_ERR_DTYPE"]
    q8.format = _lib.TFA_KV_E4M3
    assert plan(params(B=3, H=8, Hk=2, D=40, cap=1024, total_q=9), vq, ON, 1, q8)[0] == CODES["TFA_ERR_HEAD_DIM"]      # e4m3 rows are 16-element chunks


@pytest.mark.parametrize("page", [0, 128])
@pytest.mark.parametrize("B,H,Hk,D,tq", [(3, 8, 2, 64, 9), (4, 32, 8, 128, 4), (2, 16, 4, 40, 77), (2, 8, 8, 64, 6)])
def test_workspace(page, B, H, Hk, D, tq):
    L = _lib.lib()
    p, vq = params(B=B, H=H, Hk=Hk, D=D, cap=1024, total_q=tq, page=page), varlen(3, tq)
    for mode in (AUTO, ON, OFF):
        assert L.tfa_fwd_kvcache_varlen_workspace(C.byref(p), C.byref(vq), None, mode, 1) == 0
        for splits in (2, 5):
            assert L.tfa_fwd_kvcache_varlen_workspace(C.byref(p), C.byref(vq), None, mode, splits) == splits * H * tq * (D + 1)
        assert L.tfa_fwd_kvcache_varlen_workspace(C.byref(p), C.byref(vq), None, mode, 64) == 16 * H * tq * (D + 1)      # chunks never outnumber the capacity's tiles


def test_refusals_of_the_new_struct():
    L = _lib.lib()
    p = params()
    assert plan(p, None)[0] == CODES["TFA_ERR_NULL"] and plan(None, varlen())[0] == CODES["TFA_ERR_NULL"]
    v = varlen()
    v.cu_seqlens_q = None
    assert plan(p, v)[0] == CODES["TFA_ERR_NULL"]
    for kw in (dict(max_q=0), dict(max_q=-3), dict(total_q=0), dict(total_q=-1)):
        assert plan(p, varlen(**{**dict(max_q=16, total_q=64), **kw}))[0] == CODES["TFA_ERR_SHAPE"]
    for i in (0, 1):
        v = varlen()
        v.reserved_[i] = 1
        assert plan(p, v)[0] == CODES["TFA_ERR_SHAPE"]
    for off in (1, 2):
        v = varlen()
        v.cu_seqlens_q = ADDR + off
        assert plan(p, v)[0] == CODES["TFA_ERR_ALIGN"]
    # the append belongs to tfa_kvcache_append_varlen
    p = params()
    p.n_new = 1
    assert plan(p, varlen())[0] == CODES["TFA_ERR_SHAPE"]
    p = params()
    p.k_new = p.v_new = ADDR
    p.n_new = 2
    for name in ("knew_stride", "vnew_stride"):
        arr = getattr(p, name)
        arr[0], arr[1], arr[2] = 2 * 8 * 128, 128, 8 * 128
    assert plan(p, varlen())[0] == CODES["TFA_ERR_SHAPE"]
    for mode in (3, -1, 1 << 20):
        p, v = params(), varlen()
        assert plan(p, v, mode)[0] == CODES["TFA_ERR_SHAPE"]
        assert L.tfa_fwd_kvcache_varlen_workspace(C.byref(p), C.byref(v), None, mode, 2) == CODES["TFA_ERR_SHAPE"]
        assert L.tfa_fwd_kvcache_varlen(C.byref(p), C.byref(v), None, mode, 1, None, None) == CODES["TFA_ERR_SHAPE"]
        assert L.tfa_fwd_kvcache_varlen_suggest_splits(C.byref(p), C.byref(v), mode) == 1
    # Nq is not looked at
    p = params()
    p.Nq = -5
    assert plan(p, varlen())[0] == 0


@pytest.mark.parametrize("mode", [AUTO, ON, OFF])
def test_refusals_of_the_pack_plan_arrive_with_their_codes(mode):
    """Everything tfa_fwd_kvcache_pack refuses of the shared struct: the code tfa_fwd_kvcache_pack_plan gives for the same defect (there with Nq = 4)."""
    L = _lib.lib()

    def both(**kw):
        p = params(**kw)
        o = params(**kw)
        o.Nq = 4
        o.q_stride[0], o.o_stride[0] = 4 * o.H * o.D, o.H * 4 * o.D
        o.o_stride[1] = 4 * o.D
        return p, o

    cases = []
    for D in (0, 12, 136):
        cases.append(both(D=D))
    cases.append(both(dtype=_lib.TFA_F32))
    for field, val in (("q", None), ("out", None), ("k_cache", None), ("cache_seqlens", None), ("q", ADDR + 8), ("out", ADDR + 8), ("v_cache", ADDR + 8)):
        pair = both()
        for s in pair:
            setattr(s, field, val)
        cases.append(pair)
    for kw in (dict(B=0), dict(Hk=0), dict(cap=0), dict(H=12, Hk=8)):
        cases.append(both(**kw))
    pair = both(page=64)
    for s in pair:
        s.page_size = 96
    cases.append(pair)
    pair = both(page=128)
    for s in pair:
        s.block_table_stride = 4096 // 128 - 1
    cases.append(pair)
    for bad in (0.0, float("nan")):
        pair = both()
        for s in pair:
            s.softmax_scale = bad
        cases.append(pair)
    for name in ("reserved_", "reserved2_"):
        pair = both()
        for s in pair:
            setattr(s, name, 1)
        cases.append(pair)
    for name, i, val in (("q_stride", 2, 64), ("k_stride", 2, 64), ("q_stride", 1, 132), ("k_stride", 1, 132)):
        pair = both()
        for s in pair:
            getattr(s, name)[i] = val
        cases.append(pair)
    assert len(cases) > 20
    for p, o in cases:
        g = C.c_int()
        want = L.tfa_fwd_kvcache_pack_plan(C.byref(o), None, mode, 1, C.byref(g), None, None)
        assert want < 0 and plan(p, varlen(4, 64), mode)[0] == want
    assert plan(params(), varlen(), mode, 0)[0] == CODES["TFA_ERR_SHAPE"]
    # a split launch without a workspace, or with a misaligned one: refused before any launch
    p, v = params(), varlen()
    assert L.tfa_fwd_kvcache_varlen(C.byref(p), C.byref(v), None, mode, 4, None, None) == CODES["TFA_ERR_NULL"]
    assert L.tfa_fwd_kvcache_varlen(C.byref(p), C.byref(v), None, mode, 4, ADDR + 4, None) == CODES["TFA_ERR_ALIGN"]


def test_suggest_splits_hand_computed():
    """tfa_fwd_kvcache_pack_suggest_splits' rule over heads * min(B * nmb, ceil(total_q * G' / 128) + B) workgroups; 256 CUs without a device."""
    L = _lib.lib()

    def sug(mode, max_q, total_q, **kw):
        return L.tfa_fwd_kvcache_varlen_suggest_splits(C.byref(params(total_q=total_q, **kw)), C.byref(varlen(max_q, total_q)), mode)

    cus = 256
    # pure decode, one sequence: 8 workgroups packed, 32 unpacked
    assert sug(ON, 1, 1, B=1, H=32, Hk=8, cap=16384) == sug(AUTO, 1, 1, B=1, H=32, Hk=8, cap=16384) == min(32, 16384 // 1024, cus // 8) == 16
    assert sug(OFF, 1, 1, B=1, H=32, Hk=8, cap=16384) == cus // 32 == 8
    # B = 8 decode rows: min(8 * 1, ceil(8 * 4 / 128) + 8 = 9) = 8 blocks per K/V head: 64 workgroups -> 4; unpacked 256 -> 1
    assert sug(ON, 1, 8, B=8, H=32, Hk=8, cap=16384) == cus // 64 == 4 and sug(OFF, 1, 8, B=8, H=32, Hk=8, cap=16384) == 1
    # one 512-row chunk among 7 decode rows (B = 8, total_q 519): launched 8 * 16 = 128 blocks, filled at most ceil(519 * 4 / 128) + 8 = 25: 8 * 25 = 200 workgroups
    # 200 * 2 > 256 -> 1 ... and at B = 2 (total_q 513), H16 Hk4: min(2 * 16, 17 + 2 = 19) = 19 blocks * 4 K/V heads = 76 workgroups: 76 * 4 > 256 -> 2 * 256 / 76 = 6;
    # unpacked: min(2 * 4, ceil(513 / 128) + 2 = 7) = 7 blocks * 16 heads = 112: 2 * 256 / 112 = 4
    assert sug(ON, 512, 519, B=8, H=32, Hk=8, cap=16384) == 1
    assert sug(ON, 512, 513, B=2, H=16, Hk=4, cap=16384) == 2 * cus // 76 == 6
    assert sug(OFF, 512, 513, B=2, H=16, Hk=4, cap=16384) == 2 * cus // 112 == 4
    # the launch bounds the count when it is the smaller: B = 2, max_q 40 (two blocks each), total_q 80: min(4, 3 + 2) = 4 -> 32 workgroups -> 8
    assert sug(ON, 40, 80, B=2, H=32, Hk=8, cap=16384) == cus // 32 == 8
    # causal prefill: the late chunks serve few rows
    assert sug(ON, 2048, 2048, B=1, H=8, Hk=2, cap=4096, causal=True) == 1
    # short caches never split
    assert sug(ON, 1, 4, B=4, H=32, Hk=8, cap=2048) == 1
    for mode in (AUTO, ON, OFF):
        for kw in (dict(B=1), dict(B=8), dict(B=64), dict(B=3, cap=100000)):
            assert 1 <= sug(mode, 8, 64, **kw) <= 32
    assert L.tfa_fwd_kvcache_varlen_suggest_splits(None, C.byref(varlen()), ON) == 1
    assert L.tfa_fwd_kvcache_varlen_suggest_splits(C.byref(params()), None, ON) == 1


def test_existing_plans_answer_as_before():
    """The fixed-Nq entry points next to the new ones: the geometry tests/test_kvcache_packgqa_abi.py pins, and no dependence on a struct they do not take."""
    L = _lib.lib()
    p = _lib.TfaKvcacheParams()
    p.q = p.out = p.lse = p.k_cache = p.v_cache = p.cache_seqlens = ADDR
    B, H, Hk, Nq, D, cap = 3, 8, 2, 5, 64, 1024
    p.B, p.H, p.Hk, p.Nq, p.D, p.capacity = B, H, Hk, Nq, D, cap
    p.q_stride[0], p.q_stride[1], p.q_stride[2] = Nq * H * D, D, H * D
    p.o_stride[0], p.o_stride[1], p.o_stride[2] = H * Nq * D, Nq * D, D
    for name in ("k_stride", "v_stride"):
        arr = getattr(p, name)
        arr[0], arr[1], arr[2] = cap * Hk * D, D, Hk * D
    p.softmax_scale, p.is_causal, p.dtype = 0.125, 1, _lib.TFA_BF16
    g, b, l = C.c_int(), C.c_int(), C.c_int()
    for splits in (1, 2):
        assert L.tfa_fwd_kvcache_plan(C.byref(p), splits, C.byref(g), C.byref(b), C.byref(l)) == 0 and (g.value, b.value, l.value) == (B * H * splits, 256, 32768)
        assert L.tfa_fwd_kvcache_pack_plan(C.byref(p), None, ON, splits, C.byref(g), C.byref(b), C.byref(l)) == 0 and g.value == B * Hk * splits
        assert L.tfa_fwd_kvcache_pack_plan(C.byref(p), None, OFF, splits, C.byref(g), C.byref(b), C.byref(l)) == 0 and g.value == B * H * splits
        assert L.tfa_fwd_kvcache_workspace(C.byref(p), splits) == (splits * B * H * Nq * (D + 1) if splits > 1 else 0)
    p.Nq = 0
    assert L.tfa_fwd_kvcache_plan(C.byref(p), 1, C.byref(g), None, None) == CODES["TFA_ERR_SHAPE"]      # Nq is still looked at there


# ---- Python: flash_attn_with_kvcache(cu_seqlens_q=, max_seqlen_q=) against a counting stand-in for the library ---------------------------------------------
class _CountingLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a):
            self.calls.append((name, a))
            if name == "tfa_fwd_kvcache_suggest_splits":
                return 4
            if name == "tfa_fwd_kvcache_pack_suggest_splits":
                return 6
            if name == "tfa_fwd_kvcache_varlen_suggest_splits":
                return 5
            if name == "tfa_fwd_kvcache_varlen_workspace":
                p, vq, s = a[0]._obj, a[1]._obj, a[-1]
                return s * p.H * vq.total_q * (p.D + 1) if s > 1 else 0
            if name.endswith("_workspace"):
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


def _tensors(B=3, total_q=10, H=8, Hk=2, D=64, cap=1024, cache_dtype=torch.bfloat16):
    return (_meta(total_q, H, D), _meta(B, cap, Hk, D, dtype=cache_dtype), _meta(B, cap, Hk, D, dtype=cache_dtype), _meta(B, dtype=torch.int32),
            _meta(B + 1, dtype=torch.int32))


def test_wrapper_calls_the_new_entry_points(stub):
    q, kc, vc, lens, cu = _tensors()
    out, lse = ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, causal=True, return_softmax_lse=True, cu_seqlens_q=cu, max_seqlen_q=7)
    assert [c[0] for c in stub.calls] == ["tfa_fwd_kvcache_varlen_suggest_splits", "tfa_fwd_kvcache_varlen_workspace", "tfa_fwd_kvcache_varlen"]
    assert stub.calls[0][1][2] == ON                                        # None packs
    pref, vref, q8, mode, splits = stub.calls[1][1]
    assert q8 is None and mode == ON and splits == 5
    pref, vref, q8, mode, splits, ws, stream = stub.calls[2][1]
    p, v = pref._obj, vref._obj
    assert q8 is None and mode == ON and splits == 5 and ws is not None
    assert (p.B, p.H, p.Hk, p.D, p.capacity, p.is_causal, p.n_new) == (3, 8, 2, 64, 1024, 1, 0) and p.k_new is None and p.v_new is None
    assert list(p.q_stride)[1:] == [64, 8 * 64] and list(p.o_stride)[1:] == [10 * 64, 64]
    assert (v.cu_seqlens_q, v.max_seqlen_q, v.total_q, list(v.reserved_)) == (cu.data_ptr(), 7, 10, [0, 0])
    assert tuple(out.shape) == (10, 8, 64) and tuple(lse.shape) == (8, 10) and out.stride() == (64, 10 * 64, 1)      # a transposed view of the dense (H, total_q, D)
    stub.calls.clear()
    ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, num_splits=3, pack_gqa=False, cu_seqlens_q=cu, max_seqlen_q=7)
    assert [c[0] for c in stub.calls] == ["tfa_fwd_kvcache_varlen_workspace", "tfa_fwd_kvcache_varlen"] and stub.calls[-1][1][3:5] == (OFF, 3)
    stub.calls.clear()
    ops.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, num_splits=1, pack_gqa=True, cu_seqlens_q=cu, max_seqlen_q=7)
    assert stub.calls[-1][1][3:5] == (ON, 1) and stub.calls[-1][1][5] is None                         # one chunk: no workspace
    # a strided q (a slice of a packed QKV projection) hands over its own strides
    stub.calls.clear()
    qkv = _meta(10, 3, 8, 64)
    ops.flash_attn_with_kvcache(qkv[:, 0], kc, vc, cache_seqlens=lens, num_splits=1, cu_seqlens_q=cu, max_seqlen_q=7)
    assert list(stub.calls[-1][1][0]._obj.q_stride)[1:] == [64, 3 * 8 * 64]


def test_wrapper_paged_and_fp8(stub):
    q, _, _, lens, cu = _tensors()
    kp, vp = _meta(20, 128, 2, 64, dtype=torch.float8_e4m3fn), _meta(20, 128, 2, 64, dtype=torch.float8_e4m3fn)
    bt = _meta(3, 4, dtype=torch.int32)
    kd = _meta(3, 2, dtype=torch.float32)
    ops.flash_attn_with_kvcache(q, kp, vp, cache_seqlens=lens, block_table=bt, num_splits=2, k_descale=kd, cu_seqlens_q=cu, max_seqlen_q=4)
    assert [c[0] for c in stub.calls] == ["tfa_fwd_kvcache_varlen_workspace", "tfa_fwd_kvcache_varlen"]
    p, q8 = stub.calls[-1][1][0]._obj, stub.calls[-1][1][2]._obj
    assert (p.page_size, p.num_pages, p.capacity, p.block_table, p.block_table_stride) == (128, 20, 512, bt.data_ptr(), 4)
    assert q8.format == _lib.TFA_KV_E4M3 and q8.k_descale == kd.data_ptr() and q8.v_descale is None


def test_wrapper_without_cu_seqlens_q_makes_the_calls_it_made(stub):
    q4, kc, vc, lens = _meta(2, 4, 8, 64), _meta(2, 1024, 2, 64), _meta(2, 1024, 2, 64), _meta(2, dtype=torch.int32)
    ops.flash_attn_with_kvcache(q4, kc, vc, cache_seqlens=lens, causal=True)
    ops.flash_attn_with_kvcache(q4, kc, vc, cache_seqlens=lens, causal=True, num_splits=2, cu_seqlens_q=None, max_seqlen_q=None)
    ops.flash_attn_with_kvcache(q4, kc, vc, cache_seqlens=lens, pack_gqa=True)
    assert [c[0] for c in stub.calls] == ["tfa_fwd_kvcache_suggest_splits", "tfa_fwd_kvcache_workspace", "tfa_fwd_kvcache", "tfa_fwd_kvcache_workspace",
                                          "tfa_fwd_kvcache", "tfa_fwd_kvcache_pack_suggest_splits", "tfa_fwd_kvcache_pack_workspace", "tfa_fwd_kvcache_pack"]


def test_wrapper_refusals_come_before_any_library_call(stub):
    q, kc, vc, lens, cu = _tensors()
    call = lambda *a, **kw: ops.flash_attn_with_kvcache(*a, **kw)
    ok = dict(cache_seqlens=lens, cu_seqlens_q=cu, max_seqlen_q=7)
    with pytest.raises(ValueError, match="4-D q takes no cu_seqlens_q"):
        call(_meta(3, 4, 8, 64), kc, vc, **ok)
    with pytest.raises(ValueError, match="q must be a 4-D tensor"):                   # today's message, unchanged
        call(q, kc, vc, cache_seqlens=lens)
    with pytest.raises(ValueError, match="max_seqlen_q belongs to cu_seqlens_q"):
        call(_meta(3, 4, 8, 64), kc, vc, cache_seqlens=lens, max_seqlen_q=4)
    for bad in (None, 0, -2, 3.0, True, "7"):
        with pytest.raises(ValueError, match="max_seqlen_q"):
            call(q, kc, vc, cache_seqlens=lens, cu_seqlens_q=cu, max_seqlen_q=bad)
    for bad_cu in (_meta(4, dtype=torch.int64), _meta(2, 2, dtype=torch.int32), _meta(1, dtype=torch.int32), _meta(8, dtype=torch.int32)[::2], [0, 3, 6, 10]):
        with pytest.raises(ValueError, match="cu_seqlens_q"):
            call(q, kc, vc, cache_seqlens=lens, cu_seqlens_q=bad_cu, max_seqlen_q=7)
    with pytest.raises(ValueError, match="cu_seqlens_q must be contiguous and on q's device"):
        call(q, kc, vc, cache_seqlens=lens, cu_seqlens_q=torch.zeros(4, dtype=torch.int32), max_seqlen_q=7)
    # B differs between the arguments: the cache's batch, cache_seqlens, the block table, the descales
    with pytest.raises(ValueError, match="contiguous cache must have the batch size"):
        call(q, kc, vc, cache_seqlens=lens, cu_seqlens_q=_meta(6, dtype=torch.int32), max_seqlen_q=7)
    with pytest.raises(ValueError, match="cache_seqlens must be"):
        call(q, kc, vc, cache_seqlens=_meta(4, dtype=torch.int32), cu_seqlens_q=cu, max_seqlen_q=7)
    kp = _meta(20, 128, 2, 64)
    with pytest.raises(ValueError, match="block_table must be an int32 tensor of shape"):
        call(q, kp, kp, block_table=_meta(4, 4, dtype=torch.int32), **ok)
    k8 = _meta(3, 1024, 2, 64, dtype=torch.float8_e4m3fn)
    with pytest.raises(ValueError, match="k_descale must have shape"):
        call(q, k8, k8, k_descale=_meta(4, 2, dtype=torch.float32), **ok)
    # the append is another call
    with pytest.raises(ValueError, match="kvcache_append_varlen"):
        call(q, kc, vc, _meta(10, 2, 64), _meta(10, 2, 64), **ok)
    # the refusals the 4-D call has, by their names
    with pytest.raises(NotImplementedError, match="softcap"):
        call(q, kc, vc, softcap=30.0, **ok)
    with pytest.raises(NotImplementedError, match="window_size"):
        call(q, kc, vc, window_size=(128, 0), **ok)
    with pytest.raises(NotImplementedError, match="cache_leftpad"):
        call(q, kc, vc, cache_leftpad=lens, **ok)
    with pytest.raises(TypeError, match="pack_gqa"):
        call(q, kc, vc, pack_gqa="yes", **ok)
    with pytest.raises(ValueError, match="num_splits"):
        call(q, kc, vc, num_splits=-1, **ok)
    with pytest.raises(ValueError, match="head dims up to 128"):
        call(_meta(10, 8, 256), _meta(3, 1024, 2, 256), _meta(3, 1024, 2, 256), **ok)
    with pytest.raises(ValueError, match="16-byte aligned"):
        call(_meta(10, 8, 68)[:, :, :64], kc, vc, **ok)
    with pytest.raises(ValueError, match="unit stride"):
        call(_meta(10, 8, 128)[:, :, ::2], kc, vc, **ok)
    with pytest.raises(RuntimeError, match="not differentiable"):
        call(torch.empty(10, 8, 64, dtype=torch.bfloat16, device="meta", requires_grad=True), kc, vc, **ok)
    with pytest.raises(TypeError):
        ops.flash_attn_with_kvcache(q, kc, vc, None, None, lens, None, None, False, 0, False, cu)      # keyword-only
    assert stub.calls == []
