"""CPU tests of the dense-bias entry points (include/tfa.h: tfa_fwd_bias, tfa_bwd_bias and the _plan / _variant / _rounding_rule companions) and of the
``attn_bias=`` keyword of flash_attn_func / ops.flash_attn_fwd / ops.flash_attn_bwd: symbols, plans, kernel choice, rounding rule, one case per refusal code,
signature positions, and the wrappers' host-side behaviour against a recording stand-in for the library.  No GPU: plans never launch, refused calls return
before any launch, the bias is never read on the host (a stand-in address serves)."""
import ctypes as C
import inspect

import pytest
import torch

from tiny_flash_attention_amd import _lib, ops

ADDR = 0x10000          # a 16-byte aligned stand-in for device pointers (plans never dereference them)
CODES = {"TFA_ERR_NULL": -1, "TFA_ERR_DTYPE": -2, "TFA_ERR_HEAD_DIM": -3, "TFA_ERR_SHAPE": -4, "TFA_ERR_STRIDE": -5, "TFA_ERR_ALIGN": -6,
         "TFA_ERR_VARIANT": -7}
BIAS_SYMBOLS = ("tfa_fwd_bias", "tfa_fwd_bias_plan", "tfa_fwd_bias_variant", "tfa_fwd_bias_rounding_rule", "tfa_bwd_bias", "tfa_bwd_bias_plan")
WINDOWS = [(-1, -1), (-1, 0), (256, 0), (64, -1)]


def fwd_params(B=2, H=8, Hk=None, Nq=1024, Nk=1024, D=128, causal=False, dtype=_lib.TFA_BF16, out_dtype=None):
    Hk = H if Hk is None else Hk
    p = _lib.TfaFwdParams()
    p.q = p.k = p.v = p.out = p.lse = ADDR
    p.B, p.H, p.Hk, p.Nq, p.Nk, p.D = B, H, Hk, Nq, Nk, D
    for name, heads, n in (("q_stride", H, Nq), ("k_stride", Hk, Nk), ("v_stride", Hk, Nk), ("o_stride", H, Nq)):
        arr = getattr(p, name)
        arr[0], arr[1], arr[2] = heads * n * D, n * D, D
    p.softmax_scale = 0.125
    p.is_causal = 1 if causal else 0
    p.dtype = dtype
    p.out_dtype = dtype if out_dtype is None else out_dtype
    return p


def bwd_params(B=2, H=8, Hk=None, Nq=1024, Nk=1024, D=128, causal=False, dtype=_lib.TFA_BF16):
    Hk = H if Hk is None else Hk
    p = _lib.TfaBwdParams()
    for f in ("q", "k", "v", "out", "dout", "lse", "dq", "dk", "dv", "delta"):
        setattr(p, f, ADDR)
    p.B, p.H, p.Hk, p.Nq, p.Nk, p.D = B, H, Hk, Nq, Nk, D
    for name, heads, n in (("q_stride", H, Nq), ("k_stride", Hk, Nk), ("v_stride", Hk, Nk), ("o_stride", H, Nq), ("do_stride", H, Nq),
                           ("dq_stride", H, Nq), ("dk_stride", Hk, Nk), ("dv_stride", Hk, Nk)):
        arr = getattr(p, name)
        arr[0], arr[1], arr[2] = heads * n * D, n * D, D
    p.softmax_scale = 0.125
    p.is_causal = 1 if causal else 0
    p.dtype = p.grad_dtype = dtype
    return p


def bias_of(shape=(2, 8), Nq=1024, Nk=1024, dtype=_lib.TFA_BF16, ptr=ADDR, row=None):
    """A tfa_attn_bias for a dense (shape[0], shape[1], Nq, Nk) tensor (dims of size 1: stride 0)."""
    row = Nk if row is None else row
    b = _lib.TfaAttnBias()
    b.bias, b.dtype, b.reserved_ = ptr, dtype, 0
    b.stride[0] = 0 if shape[0] == 1 else shape[1] * Nq * row
    b.stride[1] = 0 if shape[1] == 1 else Nq * row
    b.stride[2] = row
    return b


def plan(p, bias, window=(-1, -1)):
    g, b, l = C.c_int(), C.c_int(), C.c_int()
    st = _lib.lib().tfa_fwd_bias_plan(C.byref(p), None if bias is None else C.byref(bias), window[0], window[1], C.byref(g), C.byref(b), C.byref(l))
    return st, g.value, b.value, l.value


def every_entry(bias, window=(-1, -1), fkw=None):
    L = _lib.lib()
    fkw = fkw or {}
    bkw = {k: v for k, v in fkw.items() if k != "out_dtype"}
    pf, pb = fwd_params(**fkw), bwd_params(**bkw)
    bp = None if bias is None else C.byref(bias)
    return {
        "fwd_plan": plan(pf, bias, window)[0],
        "fwd_variant": L.tfa_fwd_bias_variant(C.byref(pf), bp, *window),
        "fwd_rule": L.tfa_fwd_bias_rounding_rule(C.byref(pf), bp, *window),
        "bwd_plan": L.tfa_bwd_bias_plan(C.byref(pb), bp, *window),
        "fwd": L.tfa_fwd_bias(C.byref(pf), bp, window[0], window[1], None),        # (refused before any launch)
        "bwd": L.tfa_bwd_bias(C.byref(pb), bp, window[0], window[1], None),
    }


def test_symbols_exported_and_version():
    L = _lib.lib()
    for s in BIAS_SYMBOLS:
        assert s in _lib.SYMBOLS
        getattr(L, s)
    assert L.tfa_version() == 111
    assert C.sizeof(_lib.TfaAttnBias) == 40


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape", [(2, 8), (1, 8), (2, 1), (1, 1)])
@pytest.mark.parametrize("bdtype", ["q", "f32"])
def test_plan_variant_rule(window, causal, shape, bdtype):
    """Every broadcast shape, q's dtype (bf16 and f16) and fp32, every mask: accepted, the geometry tfa_fwd_alibi_plan reports for the same problem,
    variant 30 / 32, TFA_RULE_LAZY; the backward plans too."""
    L = _lib.lib()
    for qd in (_lib.TFA_BF16, _lib.TFA_F16):
        for B, H in ((2, 8), (8, 32)):
            p = fwd_params(B=B, H=H, causal=causal, dtype=qd)
            shp = (B if shape[0] != 1 else 1, H if shape[1] != 1 else 1)
            bias = bias_of(shp, dtype=qd if bdtype == "q" else _lib.TFA_F32)
            st, grid, block, lds = plan(p, bias, window)
            assert st == 0
            g, b, l = C.c_int(), C.c_int(), C.c_int()
            assert L.tfa_fwd_alibi_plan(C.byref(p), ADDR, 0, window[0], window[1], C.byref(g), C.byref(b), C.byref(l)) == 0
            assert (grid, block, lds) == (g.value, b.value, l.value)
            v = L.tfa_fwd_bias_variant(C.byref(p), C.byref(bias), *window)
            assert v in (30, 32) and v == L.tfa_fwd_alibi_variant(C.byref(p), ADDR, 0, *window)
            assert L.tfa_fwd_bias_rounding_rule(C.byref(p), C.byref(bias), *window) == _lib.RULE_LAZY
            assert L.tfa_bwd_bias_plan(C.byref(bwd_params(B=B, H=H, causal=causal, dtype=qd)), C.byref(bias), *window) == 0


@pytest.mark.parametrize("D", [40, 64, 96, 128])
def test_head_dims_gqa_and_padded_rows(D):
    """Head dims below the kernels' widths, GQA (the bias is per QUERY head), Nq != Nk and a row stride beyond Nk."""
    p = fwd_params(H=8, Hk=2, Nq=70, Nk=203, D=D)
    bias = bias_of((2, 8), Nq=70, Nk=203, row=208)
    assert plan(p, bias)[0] == 0
    assert _lib.lib().tfa_bwd_bias_plan(C.byref(bwd_params(H=8, Hk=2, Nq=70, Nk=203, D=D)), C.byref(bias), -1, -1) == 0
    one = bias_of((1, 1), Nq=70, Nk=203, row=0)                     # one row for every query (stride 0 = broadcast)
    assert plan(p, one)[0] == 0


def test_forced_variant():
    L = _lib.lib()
    bias = bias_of()
    try:
        for v in (30, 32):
            _lib.set_variant(v)
            assert L.tfa_fwd_bias_variant(C.byref(fwd_params()), C.byref(bias), -1, -1) == v
        _lib.set_variant(17)
        assert L.tfa_fwd_bias_variant(C.byref(fwd_params()), C.byref(bias), -1, -1) == CODES["TFA_ERR_VARIANT"]
        assert L.tfa_fwd_bias(C.byref(fwd_params()), C.byref(bias), -1, -1, None) == CODES["TFA_ERR_VARIANT"]
    finally:
        _lib.set_variant(-1)


def _neg_stride():
    b = bias_of()
    b.stride[0] = -b.stride[0]
    return b


def _odd_stride(i):
    b = bias_of(row=1032)
    b.stride[i] += 4
    return b


@pytest.mark.parametrize("window", [(-1, -1), (-1, 0), (256, 0)])
@pytest.mark.parametrize("make,code", [
    (lambda: None, "TFA_ERR_NULL"),                                          # NULL struct
    (lambda: bias_of(ptr=None), "TFA_ERR_NULL"),                             # NULL pointer
    (lambda: bias_of(dtype=_lib.TFA_F16), "TFA_ERR_DTYPE"),                  # a 16-bit bias that is not q's (bf16) type
    (lambda: bias_of(dtype=7), "TFA_ERR_DTYPE"),
    (lambda: bias_of(ptr=ADDR + 8), "TFA_ERR_ALIGN"),                        # base not 16-byte aligned
    (lambda: bias_of(ptr=ADDR + 2), "TFA_ERR_ALIGN"),
    (lambda: _odd_stride(0), "TFA_ERR_STRIDE"),                              # a non-zero stride that is not a multiple of 8 elements
    (lambda: _odd_stride(1), "TFA_ERR_STRIDE"),
    (lambda: _odd_stride(2), "TFA_ERR_STRIDE"),
    (_neg_stride, "TFA_ERR_STRIDE"),                                         # negative
    (lambda: bias_of(row=512), "TFA_ERR_STRIDE"),                            # rows that overlap
])
def test_bias_argument_refusals(window, make, code):
    assert set(every_entry(make(), window).values()) == {CODES[code]}


def test_refusal_slice_of_2gib():
    """A (b, h) slice of 2 GiB or more does not fit the one descriptor: fp32 32768 x 16384 is exactly 2 GiB, bf16 of the same shape half of it."""
    L = _lib.lib()
    kw = dict(B=1, H=1, Nq=32768, Nk=16384, D=64)
    big = bias_of((1, 1), Nq=32768, Nk=16384, dtype=_lib.TFA_F32)
    assert plan(fwd_params(**kw), big)[0] == CODES["TFA_ERR_STRIDE"]
    assert L.tfa_bwd_bias_plan(C.byref(bwd_params(**kw)), C.byref(big), -1, -1) == CODES["TFA_ERR_STRIDE"]
    assert plan(fwd_params(**kw), bias_of((1, 1), Nq=32768, Nk=16384))[0] == 0
    assert plan(fwd_params(**kw), bias_of((1, 1), Nq=32768, Nk=16384, row=32776))[0] == CODES["TFA_ERR_STRIDE"]   # the same rows 65552 bytes apart: 2 GiB and 240 KiB


@pytest.mark.parametrize("window", [(-1, -1), (-1, 0), (256, 0)])
@pytest.mark.parametrize("kw,code", [
    (dict(D=136), "TFA_ERR_HEAD_DIM"), (dict(D=256), "TFA_ERR_HEAD_DIM"),
    (dict(dtype=_lib.TFA_F32, out_dtype=_lib.TFA_F32), "TFA_ERR_DTYPE"),
])
def test_alibi_form_refusals(window, kw, code):
    """What the ALiBi form refuses, with its codes: head dims above 128, fp32 q."""
    assert set(every_entry(bias_of(dtype=_lib.TFA_F32), window, fkw=kw).values()) == {CODES[code]}


def test_refusal_flags_split_kv_window_and_null_params():
    L = _lib.lib()
    bias = bias_of()
    for window in ((-1, -1), (-1, 0), (256, 0)):
        p = fwd_params()
        p.flags = _lib.TFA_FWD_EXACT_MAX
        assert plan(p, bias, window)[0] == CODES["TFA_ERR_SHAPE"]
        assert L.tfa_fwd_bias_variant(C.byref(p), C.byref(bias), *window) == CODES["TFA_ERR_SHAPE"]
        p.flags = 0
        p.kv_offset = 64                                                     # split-KV / partial passes
        assert plan(p, bias, window)[0] == CODES["TFA_ERR_SHAPE"]
        p.kv_offset = 0
        p.nk_total = 2048
        assert plan(p, bias, window)[0] == CODES["TFA_ERR_SHAPE"]
    for window in ((-2, 0), (0, -2)):
        assert set(every_entry(bias, window).values()) == {CODES["TFA_ERR_SHAPE"]}
    r = bias_of()
    r.reserved_ = 1
    assert plan(fwd_params(), r)[0] == CODES["TFA_ERR_SHAPE"]
    assert L.tfa_fwd_bias_plan(None, C.byref(bias), -1, -1, None, None, None) == CODES["TFA_ERR_NULL"]
    assert L.tfa_fwd_bias(None, C.byref(bias), -1, -1, None) == CODES["TFA_ERR_NULL"]
    assert L.tfa_bwd_bias_plan(None, C.byref(bias), -1, -1) == CODES["TFA_ERR_NULL"]


def test_existing_entry_points_keep_their_rule():
    L = _lib.lib()
    p = fwd_params(B=8, H=32, Nq=4096, Nk=4096, causal=True)
    assert L.tfa_fwd_variant(C.byref(p)) == 30 and L.tfa_fwd_rounding_rule(C.byref(p)) == _lib.RULE_FIRST_TILE
    assert L.tfa_fwd_bias_rounding_rule(C.byref(p), C.byref(bias_of((8, 32), Nq=4096, Nk=4096)), -1, 0) == _lib.RULE_LAZY


# ---- Python: signatures -----------------------------------------------------------------------------------------------------------------
def test_signature_positions():
    import tiny_flash_attention_amd as tfa

    for f in (tfa.flash_attn_func, ops.flash_attn_fwd, ops.flash_attn_bwd):
        params = list(inspect.signature(f).parameters.values())
        assert [p.name for p in params[-3:]] == ["attn_bias", "softcap", "alibi_slopes"], f.__name__
        assert params[-3].kind is inspect.Parameter.KEYWORD_ONLY and params[-3].default is None
    params = list(inspect.signature(tfa.flash_attn_func).parameters.values())
    assert params[5].name == "window_size" and params[6].kind is inspect.Parameter.VAR_POSITIONAL
    params = list(inspect.signature(ops._FlashAttnBNHD.forward).parameters.values())
    assert [p.name for p in params[-4:]] == ["window_size", "attn_bias", "softcap", "alibi_slopes"]
    for f in (tfa.flash_attn_varlen_func, tfa.flash_attn_with_kvcache, ops.flash_attn_varlen_fwd, ops.flash_attn_varlen_bwd):
        assert "attn_bias" not in inspect.signature(f).parameters, f.__name__


# ---- Python: the wrappers against a recording stand-in for the library --------------------------------------------------------------------
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


B_, H_, HK_, NQ_, NK_, D_ = 2, 8, 2, 70, 208, 64


def _qkv(nq=NQ_, nk=NK_):
    return _meta(B_, H_, nq, D_), _meta(B_, HK_, nk, D_), _meta(B_, HK_, nk, D_)


def _bias_struct(call):
    return call[1][1]._obj


@pytest.mark.parametrize("shape,strides", [
    ((B_, H_), (H_ * NQ_ * NK_, NQ_ * NK_, NK_)), ((1, H_), (0, NQ_ * NK_, NK_)), ((B_, 1), (NQ_ * NK_, 0, NK_)), ((1, 1), (0, 0, NK_)),
])
@pytest.mark.parametrize("bdtype", [torch.bfloat16, torch.float32])
def test_wrapper_passes_strides_with_zero_for_broadcast_dims(stub, shape, strides, bdtype):
    q, k, v = _qkv()
    bias = _meta(shape[0], shape[1], NQ_, NK_, dtype=bdtype)
    out, lse = ops.flash_attn_fwd(q, k, v, True, None, window_size=(100, 0), attn_bias=bias)
    assert [c[0] for c in stub.calls] == ["tfa_fwd_bias"]
    name, args = stub.calls[0]
    bi = _bias_struct(stub.calls[0])
    assert tuple(bi.stride) == strides and bi.reserved_ == 0
    assert bi.dtype == (_lib.TFA_F32 if bdtype == torch.float32 else _lib.TFA_BF16)
    assert tuple(args[2:4]) == (100, 0) and args[0]._obj.is_causal == 1
    stub.calls.clear()
    ops.flash_attn_fwd(q, k, v, False, None, attn_bias=bias)                 # no mask: the window's unbounded sides
    assert stub.calls[0][0] == "tfa_fwd_bias" and tuple(stub.calls[0][1][2:4]) == (-1, -1)
    stub.calls.clear()
    ops.flash_attn_bwd(q, k, v, _meta(B_, H_, NQ_, D_), _meta(B_, H_, NQ_, dtype=torch.float32), _meta(B_, H_, NQ_, D_), True, None, attn_bias=bias)
    assert [c[0] for c in stub.calls] == ["tfa_bwd_bias"]
    assert tuple(_bias_struct(stub.calls[0]).stride) == strides and tuple(stub.calls[0][1][2:4]) == (-1, 0)


def test_wrapper_pads_rows_that_miss_the_alignment(stub):
    """Nk = 203: the rows of a dense bias are 203 elements apart — one padded copy, row stride 208; an expanded (stride-0) bias needs none."""
    q, k, v = _qkv(nk=203)
    bias = _meta(B_, H_, NQ_, 203)
    ops.flash_attn_fwd(q, k, v, False, None, attn_bias=bias)
    bi = _bias_struct(stub.calls[0])
    assert tuple(bi.stride) == (H_ * NQ_ * 208, NQ_ * 208, 208)
    stub.calls.clear()
    ops.flash_attn_fwd(q, k, v, False, None, attn_bias=_meta(1, 1, NQ_, 203))
    assert tuple(_bias_struct(stub.calls[0]).stride) == (0, 0, 208)
    stub.calls.clear()
    sliced = _meta(B_, H_, NQ_, 256)[..., :203]                              # already a padded buffer: passed as it is
    ops.flash_attn_fwd(q, k, v, False, None, attn_bias=sliced)
    assert tuple(_bias_struct(stub.calls[0]).stride) == (H_ * NQ_ * 256, NQ_ * 256, 256)
    stub.calls.clear()
    ops.flash_attn_fwd(q, k, v, False, None, attn_bias=_meta(1, H_, NQ_, 203).expand(B_, H_, NQ_, 203)[..., :203])
    assert tuple(_bias_struct(stub.calls[0]).stride)[0] == 0


def test_bool_mask_becomes_zero_or_minus_inf_in_q_dtype():
    """SDPA's convention: True = attend.  On the CPU (the helper never reads a device): 0 where True, -inf where False, q's dtype."""
    cpu = torch.device("cpu")
    g = torch.Generator().manual_seed(0)
    m = torch.rand(1, 2, 5, 16, generator=g) < 0.5
    for dt in (torch.bfloat16, torch.float16):
        t, bi = ops._attn_bias(m, 3, 2, 5, 16, cpu, dt, 64)
        assert t.dtype == dt and tuple(t.shape) == (1, 2, 5, 16)
        assert bool((t[m] == 0).all()) and bool(torch.isneginf(t[~m]).all())
        assert bi.dtype == (_lib.TFA_BF16 if dt == torch.bfloat16 else _lib.TFA_F16) and tuple(bi.stride) == (0, 5 * 16, 16)
    assert ops._attn_bias(None, 3, 2, 5, 16, cpu, torch.float32, 256) is None      # no bias: nothing is checked


def test_padded_copy_keeps_the_values():
    cpu = torch.device("cpu")
    b = torch.arange(2 * 3 * 11, dtype=torch.float32).view(1, 2, 3, 11)
    t, bi = ops._attn_bias(b, 4, 2, 3, 11, cpu, torch.bfloat16, 64)
    assert torch.equal(t, b) and t.stride(2) == 16 and tuple(bi.stride) == (0, 3 * 16, 16) and bi.dtype == _lib.TFA_F32


def test_python_refusals_happen_before_any_library_call(stub):
    import tiny_flash_attention_amd as tfa

    q, k, v = _meta(B_, NQ_, H_, D_), _meta(B_, NK_, HK_, D_), _meta(B_, NK_, HK_, D_)      # (B, N, H, D) for flash_attn_func
    ok = _meta(B_, H_, NQ_, NK_)
    f = tfa.flash_attn_func
    for bad in ([0.0], 1.0):
        with pytest.raises(TypeError, match="tensor"):
            f(q, k, v, attn_bias=bad)
    for dt in (torch.float64, torch.int32, torch.float16, torch.uint8):
        with pytest.raises(TypeError, match="dtype"):
            f(q, k, v, attn_bias=_meta(B_, H_, NQ_, NK_, dtype=dt))
    for shape in ((NQ_, NK_), (H_, NQ_, NK_), (B_, H_, NQ_, NK_ + 1), (B_, H_, NQ_ + 1, NK_), (3, H_, NQ_, NK_), (B_, HK_, NQ_, NK_), (B_, H_, 1, NK_),
                  (1, B_, H_, NQ_, NK_)):
        with pytest.raises(ValueError, match="shape"):
            f(q, k, v, attn_bias=_meta(*shape))
    with pytest.raises(ValueError, match="device"):
        f(q, k, v, attn_bias=torch.zeros(B_, H_, NQ_, NK_, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="alibi_slopes"):
        f(q, k, v, attn_bias=ok, alibi_slopes=_meta(H_, dtype=torch.float32))
    with pytest.raises(ValueError, match="softcap"):
        f(q, k, v, attn_bias=ok, softcap=30.0)
    with pytest.raises(RuntimeError, match="requires grad"):
        f(q, k, v, attn_bias=_meta(B_, H_, NQ_, NK_).requires_grad_(True))
    with pytest.raises(RuntimeError, match="requires grad"):
        f(_meta(B_, NQ_, H_, D_).requires_grad_(True), k, v, attn_bias=_meta(B_, H_, NQ_, NK_, dtype=torch.float32).requires_grad_(True))
    qb, kb, vb = _qkv()
    with pytest.raises(ValueError, match="float16 / bfloat16"):
        ops.flash_attn_fwd(*(t.float() for t in (qb, kb, vb)), False, None, attn_bias=_meta(B_, H_, NQ_, NK_, dtype=torch.float32))
    with pytest.raises(ValueError, match="up to 128"):
        ops.flash_attn_fwd(_meta(B_, H_, NQ_, 256), _meta(B_, HK_, NK_, 256), _meta(B_, HK_, NK_, 256), False, None, attn_bias=ok)
    with pytest.raises(ValueError, match="exact_max"):
        ops.flash_attn_fwd(qb, kb, vb, False, None, exact_max=True, attn_bias=ok)
    with pytest.raises(ValueError, match="split-KV"):
        ops.flash_attn_fwd(qb, kb, vb, False, None, kv_offset=64, nk_total=1024, attn_bias=ok)
    with pytest.raises(ValueError, match="dS-workspace"):
        ops.flash_attn_bwd(qb, kb, vb, _meta(B_, H_, NQ_, D_), _meta(B_, H_, NQ_, dtype=torch.float32), _meta(B_, H_, NQ_, D_), False, None, workspace=True,
                           attn_bias=ok)
    assert stub.calls == []
    with pytest.raises(TypeError):
        tfa.flash_attn_varlen_func(_meta(4, 2, 64), _meta(4, 2, 64), _meta(4, 2, 64), _meta(2, dtype=torch.int32), _meta(2, dtype=torch.int32), 4, 4,
                                   attn_bias=ok)
    with pytest.raises(TypeError):
        tfa.flash_attn_with_kvcache(_meta(1, 1, 2, 64), _meta(1, 64, 2, 64), _meta(1, 64, 2, 64), attn_bias=ok)
    assert stub.calls == []


def test_without_a_bias_the_call_is_todays(stub):
    """attn_bias=None (given or not): exactly the library calls the functions made before the keyword existed, with the same arguments."""
    import tiny_flash_attention_amd as tfa

    q, k, v = _meta(B_, NQ_, H_, D_), _meta(B_, NK_, HK_, D_), _meta(B_, NK_, HK_, D_)
    slopes = _meta(H_, dtype=torch.float32)
    seen = []
    for kw in ({}, {"attn_bias": None}):
        for args, name in ((dict(), "tfa_fwd"), (dict(causal=True), "tfa_fwd"), (dict(window_size=(16, 0)), "tfa_fwd_local"),
                           (dict(alibi_slopes=slopes), "tfa_fwd_alibi"), (dict(softcap=30.0), "tfa_fwd_softcap")):
            stub.calls.clear()
            tfa.flash_attn_func(q, k, v, **args, **kw)
            assert [c[0] for c in stub.calls] == [name]
            p = stub.calls[0][1][0]._obj
            rest = tuple(a for a in stub.calls[0][1][1:] if not isinstance(a, C.c_void_p))
            seen.append((name, rest, (p.q, p.k, p.v, p.B, p.H, p.Hk, p.Nq, p.Nk, p.D, list(p.q_stride), list(p.k_stride), list(p.v_stride), list(p.o_stride),
                                      p.is_causal, p.dtype, p.out_dtype, p.softmax_scale, p.flags)))
    assert seen[:5] == seen[5:]
    qb, kb, vb = _qkv()
    for kw in ({}, {"attn_bias": None}):
        stub.calls.clear()
        ops.flash_attn_bwd(qb, kb, vb, _meta(B_, H_, NQ_, D_), _meta(B_, H_, NQ_, dtype=torch.float32), _meta(B_, H_, NQ_, D_), True, None, **kw)
        assert [c[0] for c in stub.calls] == ["tfa_bwd"]
    stub.calls.clear()
    qg = _meta(B_, NQ_, H_, D_).requires_grad_(True)
    tfa.flash_attn_func(qg, k, v, causal=True, attn_bias=None)
    assert [c[0] for c in stub.calls] == ["tfa_fwd"]
    stub.calls.clear()
    tfa.flash_attn_func(qg, k, v, causal=True, attn_bias=_meta(1, 1, NQ_, NK_))
    assert [c[0] for c in stub.calls] == ["tfa_fwd_bias"] and tuple(stub.calls[0][1][2:4]) == (-1, 0)
