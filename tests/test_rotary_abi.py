"""CPU tests of the rotary entry points (include/tfa.h: tfa_rotary, tfa_rotary_plan) and of the Python wrappers ``apply_rotary_emb`` / ``apply_rotary_emb_qk_``:
symbols, struct size, plans and their grids, one case per refusal code, and the wrappers' host-side behaviour against a counting stand-in for the library.
No GPU: plans never launch, refused calls return before any launch, the offsets and cu_seqlens are never read on the host (a stand-in address serves)."""
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
ROTARY_SYMBOLS = ("tfa_rotary", "tfa_rotary_plan")


def params(B=2, N=5, H=3, D=64, rd=64, ro=128, H2=0, packed=False, interleaved=False, dtype=_lib.TFA_BF16, cs_dtype=None, inplace=False, dev_offsets=False):
    """A tfa_rotary_params over contiguous (B, N, H, D) — or packed (N, H, D) — tensors and contiguous tables."""
    p = _lib.TfaRotaryParams()
    p.x = ADDR
    p.out = ADDR if inplace else 2 * ADDR
    p.cos, p.sin = 3 * ADDR, 4 * ADDR
    p.B, p.N, p.H, p.H2, p.D, p.rotary_dim, p.seqlen_ro = B, N, H, H2, D, rd, ro
    for name, h in (("x_stride", H), ("o_stride", H)) + ((("x2_stride", H2), ("o2_stride", H2)) if H2 else ()):
        arr = getattr(p, name)
        arr[0], arr[1], arr[2] = (0 if packed else N * h * D), D, h * D
    if H2:
        p.x2 = 5 * ADDR
        p.out2 = 5 * ADDR if inplace else 6 * ADDR
    if packed:
        p.cu_seqlens = 7 * ADDR
    if dev_offsets:
        p.seqlen_offsets = 8 * ADDR
    p.cos_stride = p.sin_stride = rd // 2
    p.dtype = dtype
    p.cs_dtype = dtype if cs_dtype is None else cs_dtype
    p.interleaved = 1 if interleaved else 0
    return p


def plan(p):
    g, b = C.c_int(), C.c_int()
    return _lib.lib().tfa_rotary_plan(C.byref(p), C.byref(g), C.byref(b)), g.value, b.value


def test_symbols_exported_and_version():
    L = _lib.lib()
    for s in ROTARY_SYMBOLS:
        assert s in _lib.SYMBOLS
        getattr(L, s)
    assert L.tfa_version() == 111


def test_struct_size_matches_the_header():
    src = '#include <stdio.h>\n#include "tfa.h"\nint main(void) { printf("%zu", sizeof(tfa_rotary_params)); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.check_call(["cc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        assert int(subprocess.check_output([exe]).decode()) == C.sizeof(_lib.TfaRotaryParams)


@pytest.mark.parametrize("D,rd", [(64, 64), (128, 32), (40, 16), (128, 128)])
@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("H2", [0, 1])
def test_plan_grid_counts_the_work_items(D, rd, interleaved, H2):
    """One item per (row, head, pair of chunks) in the GPT-NeoX layout — rd / 16 pairs plus the copied chunks —, per chunk in the GPT-J layout; 256 threads a block."""
    items = D // 8 if interleaved else rd // 16 + (D - rd) // 8
    for B, N, packed in ((2, 70, False), (4, 73, True), (1, 1, False)):
        rows = N if packed else B * N
        for dtype in (_lib.TFA_BF16, _lib.TFA_F16):
            for cs in (dtype, _lib.TFA_F32):
                st, grid, block = plan(params(B=B, N=N, D=D, rd=rd, H2=H2, packed=packed, interleaved=interleaved, dtype=dtype, cs_dtype=cs))
                assert (st, grid, block) == (0, -(-rows * (3 + H2) * items // 256), 256)
    assert plan(params(D=D, rd=rd, H2=H2, interleaved=interleaved, inplace=True, dev_offsets=True))[0] == 0


@pytest.mark.parametrize("field", ["x", "out", "cos", "sin", "x2", "out2"])
def test_refusal_null(field):
    p = params(H2=1)
    setattr(p, field, None)
    assert plan(p)[0] == CODES["TFA_ERR_NULL"]
    assert _lib.lib().tfa_rotary(C.byref(p), None) == CODES["TFA_ERR_NULL"]


def test_refusal_null_params():
    assert _lib.lib().tfa_rotary_plan(None, None, None) == CODES["TFA_ERR_NULL"]
    assert _lib.lib().tfa_rotary(None, None) == CODES["TFA_ERR_NULL"]


@pytest.mark.parametrize("kw", [dict(dtype=_lib.TFA_F32), dict(dtype=7), dict(cs_dtype=_lib.TFA_F16), dict(cs_dtype=9)])
def test_refusal_dtype(kw):
    assert plan(params(**kw))[0] == CODES["TFA_ERR_DTYPE"]          # (the default x is bf16: f16 tables are neither x's dtype nor fp32)


@pytest.mark.parametrize("D,rd", [(0, 16), (4, 16), (60, 16), (64, 0), (64, 8), (64, 24), (64, 80), (40, 48), (64, -16)])
def test_refusal_head_dim(D, rd):
    p = params()
    p.D, p.rotary_dim = D, rd
    assert plan(p)[0] == CODES["TFA_ERR_HEAD_DIM"]


@pytest.mark.parametrize("kw", [dict(B=0), dict(N=0), dict(H=0), dict(ro=0), dict(B=-1)])
def test_refusal_shapes(kw):
    assert plan(params(**kw))[0] == CODES["TFA_ERR_SHAPE"]


def test_refusal_second_tensor_and_flags():
    p = params(H2=1)
    p.H2 = 0                                        # a second tensor without heads
    assert plan(p)[0] == CODES["TFA_ERR_SHAPE"]
    p = params()
    p.H2 = 2                                        # heads without a tensor
    assert plan(p)[0] == CODES["TFA_ERR_SHAPE"]
    for field in ("interleaved", "conjugate"):
        p = params()
        setattr(p, field, 2)
        assert plan(p)[0] == CODES["TFA_ERR_SHAPE"]
    p = params(B=1 << 20, N=1 << 10, H=128, D=256, rd=256, interleaved=True)      # 2^42 items: a grid of 2^34 blocks
    assert plan(p)[0] == CODES["TFA_ERR_SHAPE"]


@pytest.mark.parametrize("name", ["x_stride", "o_stride", "x2_stride", "o2_stride"])
def test_refusal_strides(name):
    p = params(H2=1)
    getattr(p, name)[0] = -64
    assert plan(p)[0] == CODES["TFA_ERR_STRIDE"]
    p = params(H2=1)
    getattr(p, name)[1] = 68                        # a head 136 bytes on: chunks no longer 16-byte aligned
    assert plan(p)[0] == CODES["TFA_ERR_STRIDE"]
    p = params(H2=1, packed=True)
    getattr(p, name)[0] = -64                       # packed: the batch stride is not looked at
    assert plan(p)[0] == 0


def test_refusal_table_strides_and_inplace_strides():
    for field in ("cos_stride", "sin_stride"):
        p = params(rd=32)
        setattr(p, field, 8)                        # rows overlap (16 values each)
        assert plan(p)[0] == CODES["TFA_ERR_STRIDE"]
        p = params(rd=32)
        setattr(p, field, 20)                       # bf16 rows 40 bytes apart
        assert plan(p)[0] == CODES["TFA_ERR_STRIDE"]
        p = params(rd=32, cs_dtype=_lib.TFA_F32)
        setattr(p, field, 20)                       # fp32 rows 80 bytes apart: fine
        assert plan(p)[0] == 0
    p = params(inplace=True)
    p.o_stride[2] = 2 * p.x_stride[2]               # out == x read by other strides
    assert plan(p)[0] == CODES["TFA_ERR_STRIDE"]


@pytest.mark.parametrize("field,off", [("x", 8), ("out", 8), ("x2", 8), ("out2", 8), ("cos", 8), ("sin", 4), ("seqlen_offsets", 2), ("cu_seqlens", 2)])
def test_refusal_alignment(field, off):
    p = params(H2=1, packed=True, dev_offsets=True)
    setattr(p, field, getattr(p, field) + off)
    assert plan(p)[0] == CODES["TFA_ERR_ALIGN"]


def test_header_still_compiles_as_plain_c():
    src = '#include "tfa.h"\nint main(void) { tfa_rotary_params p; (void)p; (void)tfa_rotary; (void)tfa_rotary_plan; return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "h.c")
        open(c, "w").write(src)
        subprocess.check_call(["cc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", c, "-o", os.path.join(d, "h.o")])


# ---- Python: the wrappers against a counting stand-in for the library ----------------------------------------------------------------------
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


def test_wrappers_are_exported():
    import tiny_flash_attention_amd as tfa

    for n in ("apply_rotary_emb", "apply_rotary_emb_qk_"):
        assert getattr(tfa, n) is getattr(ops, n) and n in tfa.__all__


def test_wrapper_takes_a_slice_of_a_packed_projection_without_a_copy(stub):
    B, N, H, D, rd, ro = 2, 7, 4, 64, 32, 100
    qkv = _meta(B, N, 3, H, D)
    x = qkv[:, :, 1]
    cos, sin = _meta(ro, rd // 2), _meta(ro, rd // 2)
    out = ops.apply_rotary_emb(x, cos, sin)
    assert [c[0] for c in stub.calls] == ["tfa_rotary"]
    p = stub.calls[0][1][0]._obj
    assert p.x == _ptr(qkv) + H * D * 2 and p.out == _ptr(out) and p.x2 is None and p.out2 is None
    assert (p.B, p.N, p.H, p.H2, p.D, p.rotary_dim, p.seqlen_ro) == (B, N, H, 0, D, rd, ro)
    assert list(p.x_stride) == [N * 3 * H * D, D, 3 * H * D] and list(p.o_stride) == [N * H * D, D, H * D]
    assert (p.cos, p.sin, p.cos_stride, p.sin_stride) == (_ptr(cos), _ptr(sin), rd // 2, rd // 2)
    assert (p.dtype, p.cs_dtype, p.interleaved, p.conjugate) == (_lib.TFA_BF16, _lib.TFA_BF16, 0, 0)
    assert p.seqlen_offsets is None and p.seqlen_offset == 0 and p.cu_seqlens is None
    assert out.shape == x.shape and out.is_contiguous()


def test_wrapper_fp32_tables_host_and_device_offsets_inplace(stub):
    B, N, H, D, rd, ro = 3, 1, 2, 128, 128, 64
    x = _meta(B, N, H, D, dtype=torch.float16)
    cos, sin = _meta(ro, rd // 2, dtype=torch.float32), _meta(ro, rd // 2, dtype=torch.float32)
    assert ops.apply_rotary_emb(x, cos, sin, interleaved=True, inplace=True, seqlen_offsets=17) is x
    p = stub.calls[-1][1][0]._obj
    assert p.out == p.x == _ptr(x) and list(p.o_stride) == list(p.x_stride)
    assert (p.dtype, p.cs_dtype, p.interleaved, p.conjugate) == (_lib.TFA_F16, _lib.TFA_F32, 1, 0)
    assert p.seqlen_offsets is None and p.seqlen_offset == 17
    lens = _meta(B, dtype=torch.int32)
    ops.apply_rotary_emb(x, cos, sin, seqlen_offsets=lens, max_seqlen=5)
    p = stub.calls[-1][1][0]._obj
    assert p.seqlen_offsets == _ptr(lens) and p.seqlen_offset == 0 and p.out != p.x
    ops.apply_rotary_emb(x, cos, sin, seqlen_offsets=-3)
    assert stub.calls[-1][1][0]._obj.seqlen_offset == -3
    assert len(stub.calls) == 3


def test_wrapper_makes_a_misaligned_table_contiguous_once(stub):
    x = _meta(1, 4, 2, 64)
    wide = _meta(50, 40)                            # rows 80 bytes apart, the view starts 8 bytes in
    cos, sin = wide[:, 4:20], _meta(50, 16)
    ops.apply_rotary_emb(x, cos, sin)
    p = stub.calls[-1][1][0]._obj
    assert p.cos_stride == 16 and p.cos % 16 == 0 and p.cos != _ptr(cos)
    assert p.sin == _ptr(sin) and p.sin_stride == 16
    ok = _meta(50, 64)[:, :16]                      # rows 128 bytes apart from an aligned base: used as it is
    ops.apply_rotary_emb(x, ok, ok)
    p = stub.calls[-1][1][0]._obj
    assert p.cos == _ptr(ok) and p.cos_stride == 64


def test_wrapper_packed_form_and_the_pair_call(stub):
    total, H, Hk, D, B = 20, 8, 2, 64, 4
    qkv = _meta(total, H + 2 * Hk, D)
    q, k = qkv[:, :H], qkv[:, H:H + Hk]
    cos = _meta(64, 32)
    cu, lens = _meta(B + 1, dtype=torch.int32), _meta(B, dtype=torch.int32)
    rq, rk = ops.apply_rotary_emb_qk_(q, k, cos, cos, seqlen_offsets=lens, cu_seqlens=cu)
    assert rq is q and rk is k and [c[0] for c in stub.calls] == ["tfa_rotary"]       # ONE launch
    p = stub.calls[0][1][0]._obj
    assert (p.x, p.out, p.x2, p.out2) == (_ptr(q), _ptr(q), _ptr(k), _ptr(k)) and p.x2 == p.x + H * D * 2
    assert (p.B, p.N, p.H, p.H2, p.D) == (B, total, H, Hk, D)
    row = (H + 2 * Hk) * D
    assert list(p.x_stride) == [0, D, row] == list(p.o_stride) and list(p.x2_stride) == [0, D, row] == list(p.o2_stride)
    assert p.cu_seqlens == _ptr(cu) and p.seqlen_offsets == _ptr(lens) and p.conjugate == 0
    out = ops.apply_rotary_emb(q, cos, cos, cu_seqlens=cu, max_seqlen=9)
    p = stub.calls[-1][1][0]._obj
    assert (p.B, p.N, p.H, p.H2) == (B, total, H, 0) and p.x2 is None and tuple(out.shape) == (total, H, D)


def test_wrappers_refuse_by_name_before_any_call(stub):
    f, g = ops.apply_rotary_emb, ops.apply_rotary_emb_qk_
    x, cos = _meta(2, 5, 3, 64), _meta(32, 32)
    i32 = lambda *s: _meta(*s, dtype=torch.int32)
    with pytest.raises(TypeError, match="x must be a tensor"):
        f([1.0], cos, cos)
    with pytest.raises(TypeError, match="cos must be a tensor"):
        f(x, None, cos)
    with pytest.raises(TypeError, match="sin must be a tensor"):
        f(x, cos, 3)
    for dt in (torch.float32, torch.float8_e4m3fn):
        with pytest.raises(TypeError, match="float16 or bfloat16"):
            f(_meta(2, 5, 3, 64, dtype=dt), cos, cos)
    with pytest.raises(ValueError, match="4-D"):
        f(_meta(5, 3, 64), cos, cos)
    with pytest.raises(ValueError, match="3-D"):
        f(x, cos, cos, cu_seqlens=i32(3))
    with pytest.raises(ValueError, match="2-D"):
        f(x, _meta(32), _meta(32))
    with pytest.raises(ValueError, match="multiple of 16"):
        f(x, _meta(32, 12), _meta(32, 12))
    with pytest.raises(ValueError, match="exceed the head dim"):
        f(x, _meta(32, 40), _meta(32, 40))
    with pytest.raises(ValueError, match="multiple of 8"):
        f(_meta(2, 5, 3, 36), _meta(32, 8), _meta(32, 8))
    with pytest.raises(ValueError, match="one shape and dtype"):
        f(x, cos, _meta(31, 32))
    with pytest.raises(ValueError, match="one shape and dtype"):
        f(x, cos, _meta(32, 32, dtype=torch.float32))
    with pytest.raises(ValueError, match="x's dtype"):
        f(x, _meta(32, 32, dtype=torch.float16), _meta(32, 32, dtype=torch.float16))
    with pytest.raises(ValueError, match="unit stride"):
        f(_meta(2, 5, 64, 3).transpose(2, 3), cos, cos)
    for bad in (i32(3), _meta(2, dtype=torch.int64), i32(2, 1), i32(4)[::2], 1.5, None, torch.empty(2, dtype=torch.int32)):
        with pytest.raises(ValueError, match="seqlen_offsets"):
            f(x, cos, cos, seqlen_offsets=bad)
    xp = _meta(10, 3, 64)
    for bad in (_meta(3, dtype=torch.int64), i32(3, 1), i32(1), i32(6)[::2], [0, 5, 10], torch.empty(3, dtype=torch.int32)):
        with pytest.raises(ValueError, match="cu_seqlens"):
            f(xp, cos, cos, cu_seqlens=bad)
    k = _meta(2, 5, 1, 64)
    with pytest.raises(TypeError, match="k must be a tensor"):
        g(x, None, cos, cos)
    with pytest.raises(ValueError, match="one dtype and device"):
        g(x, _meta(2, 5, 1, 64, dtype=torch.float16), cos, cos)
    with pytest.raises(ValueError, match="head count"):
        g(x, _meta(2, 6, 1, 64), cos, cos)
    with pytest.raises(ValueError, match="head count"):
        g(x, _meta(2, 5, 1, 128), cos, cos)
    with pytest.raises(RuntimeError, match="inference-only"):
        g(x, _meta(2, 5, 1, 64).requires_grad_(True), cos, cos)
    assert g(x, k, cos, cos)[1] is k and len(stub.calls) == 1
    stub.calls.clear()
    with pytest.raises(ValueError, match="seqlen_offsets"):
        g(x, k, cos, cos, seqlen_offsets=i32(5))
    assert stub.calls == []
