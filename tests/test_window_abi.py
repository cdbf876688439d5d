"""CPU tests of the local (sliding-window) entry points (include/tfa.h: tfa_fwd_local, tfa_bwd_local and their varlen forms): symbols, plans,
kernel choice, rounding rule, refusal codes and the Python wrappers' host-side rejections.  No GPU: plans never launch, refused calls return before
any launch, and the wrappers refuse before they touch a device."""
import ctypes as C

import pytest
import torch

from tiny_flash_attention_amd import _lib, ops

ADDR = 0x10000          # a 16-byte aligned stand-in for device pointers (plans never dereference them)
CODES = {"TFA_ERR_NULL": -1, "TFA_ERR_DTYPE": -2, "TFA_ERR_HEAD_DIM": -3, "TFA_ERR_SHAPE": -4, "TFA_ERR_STRIDE": -5, "TFA_ERR_VARIANT": -7}
LOCAL_SYMBOLS = ("tfa_fwd_local", "tfa_fwd_local_plan", "tfa_fwd_local_variant", "tfa_fwd_local_rounding_rule",
                 "tfa_fwd_varlen_local", "tfa_fwd_varlen_local_plan", "tfa_fwd_varlen_local_variant", "tfa_fwd_varlen_local_rounding_rule",
                 "tfa_bwd_local", "tfa_bwd_local_plan", "tfa_bwd_varlen_local", "tfa_bwd_varlen_local_plan")


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


def varlen_params(B=4, H=8, Hk=8, D=128, max_q=1024, max_k=1024, total_q=4096, total_k=4096, causal=False, dtype=_lib.TFA_BF16):
    p = _lib.TfaVarlenFwdParams()
    p.q = p.k = p.v = p.out = p.lse = p.cu_seqlens_q = p.cu_seqlens_k = ADDR
    p.B, p.H, p.Hk, p.D = B, H, Hk, D
    p.max_seqlen_q, p.max_seqlen_k, p.total_q, p.total_k = max_q, max_k, total_q, total_k
    for name, heads in (("q_stride", H), ("k_stride", Hk), ("v_stride", Hk), ("o_stride", H)):
        arr = getattr(p, name)
        arr[0], arr[1] = D, heads * D
    p.softmax_scale = 0.125
    p.is_causal = 1 if causal else 0
    p.dtype = p.out_dtype = dtype
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


def plan(p, left, right):
    g, b, l = C.c_int(), C.c_int(), C.c_int()
    return _lib.lib().tfa_fwd_local_plan(C.byref(p), left, right, C.byref(g), C.byref(b), C.byref(l)), g.value, b.value


def test_symbols_exported():
    L = _lib.lib()
    for s in LOCAL_SYMBOLS:
        assert s in _lib.SYMBOLS
        getattr(L, s)


@pytest.mark.parametrize("window", [(256, 0), (0, 0), (128, 128), (0, 300), (-1, 64), (64, -1), (1000, 0)])
@pytest.mark.parametrize("B,H", [(2, 8), (8, 32)])
def test_plan_variant_rule(window, B, H):
    p = fwd_params(B=B, H=H)
    st, grid, block = plan(p, *window)
    assert st == 0
    v = _lib.lib().tfa_fwd_local_variant(C.byref(p), *window)
    assert v in (30, 32)
    bm, wg = (256, 512) if v == 30 else (128, 256)
    assert block == wg and grid == B * H * ((1024 + bm - 1) // bm)     # one query block per work item: no causal pairs
    assert _lib.lib().tfa_fwd_local_rounding_rule(C.byref(p), *window) == _lib.RULE_LAZY
    pv = varlen_params(B=B, H=H)
    g, b_, l_ = C.c_int(), C.c_int(), C.c_int()
    assert _lib.lib().tfa_fwd_varlen_local_plan(C.byref(pv), window[0], window[1], C.byref(g), C.byref(b_), C.byref(l_)) == 0
    assert _lib.lib().tfa_fwd_varlen_local_variant(C.byref(pv), *window) in (30, 32)
    assert _lib.lib().tfa_fwd_varlen_local_rounding_rule(C.byref(pv), *window) == _lib.RULE_LAZY
    assert _lib.lib().tfa_bwd_local_plan(C.byref(bwd_params(B=B, H=H)), *window) == 0


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D,dtype", [(128, _lib.TFA_BF16), (64, _lib.TFA_F16), (256, _lib.TFA_BF16), (96, _lib.TFA_F16)])
@pytest.mark.parametrize("B,H,N", [(2, 8, 1024), (8, 32, 4096), (1, 4, 300)])
def test_full_and_causal_windows_are_tfa_fwd(causal, D, dtype, B, H, N):
    """(-1, -1) / (-1, 0) report what tfa_fwd reports with is_causal 0 / 1 — the same kernel, plan and rounding rule."""
    L = _lib.lib()
    for window, c in (((-1, -1), causal), ((-1, 0), True), ((N + 10, 0), True)):
        p = fwd_params(B=B, H=H, Nq=N, Nk=N, D=D, causal=causal, dtype=dtype)
        ref = fwd_params(B=B, H=H, Nq=N, Nk=N, D=D, causal=c, dtype=dtype)
        assert L.tfa_fwd_local_variant(C.byref(p), *window) == L.tfa_fwd_variant(C.byref(ref))
        assert L.tfa_fwd_local_rounding_rule(C.byref(p), *window) == L.tfa_fwd_rounding_rule(C.byref(ref))
        g0, b0, l0 = C.c_int(), C.c_int(), C.c_int()
        assert L.tfa_fwd_plan(C.byref(ref), C.byref(g0), C.byref(b0), C.byref(l0)) == 0
        st, grid, block = plan(p, *window)
        assert st == 0 and (grid, block) == (g0.value, b0.value)


def test_causal_forces_right_zero():
    L = _lib.lib()
    p = fwd_params(causal=True)
    # (-1, 300) under causal is plain causal attention; (64, 300) is the (64, 0) window
    assert L.tfa_fwd_local_variant(C.byref(p), -1, 300) == L.tfa_fwd_variant(C.byref(fwd_params(causal=True)))
    assert plan(p, 64, 300)[1:] == plan(fwd_params(), 64, 0)[1:]


def test_forced_variant():
    L = _lib.lib()
    try:
        for v in (30, 32):
            _lib.set_variant(v)
            assert L.tfa_fwd_local_variant(C.byref(fwd_params()), 256, 0) == v
        _lib.set_variant(36)
        assert L.tfa_fwd_local_variant(C.byref(fwd_params()), 256, 0) == CODES["TFA_ERR_VARIANT"]
    finally:
        _lib.set_variant(-1)


@pytest.mark.parametrize("kw,window,code", [
    (dict(D=136), (256, 0), "TFA_ERR_HEAD_DIM"), (dict(D=256), (256, 0), "TFA_ERR_HEAD_DIM"),
    (dict(dtype=_lib.TFA_F32, out_dtype=_lib.TFA_F32), (256, 0), "TFA_ERR_DTYPE"),
    (dict(), (-2, 0), "TFA_ERR_SHAPE"), (dict(), (0, -2), "TFA_ERR_SHAPE"), (dict(), (-5, -5), "TFA_ERR_SHAPE"),
])
def test_refusals(kw, window, code):
    L = _lib.lib()
    want = CODES[code]
    p = fwd_params(**kw)
    assert plan(p, *window)[0] == want
    assert L.tfa_fwd_local_variant(C.byref(p), *window) == want
    assert L.tfa_fwd_local(C.byref(p), window[0], window[1], None) == want
    vkw = {k: v for k, v in kw.items() if k in ("D", "dtype")}
    pv = varlen_params(**vkw)
    if "out_dtype" in kw:
        pv.out_dtype = kw["out_dtype"]
    assert L.tfa_fwd_varlen_local_variant(C.byref(pv), *window) == want
    bkw = {k: v for k, v in kw.items() if k in ("D", "dtype")}
    assert L.tfa_bwd_local_plan(C.byref(bwd_params(**bkw)), *window) == want


def test_refusal_flags():
    L = _lib.lib()
    p = fwd_params()
    p.flags = _lib.TFA_FWD_EXACT_MAX
    assert plan(p, 256, 0)[0] == CODES["TFA_ERR_SHAPE"]
    p.flags = 0
    p.kv_offset = 64
    assert plan(p, 256, 0)[0] == CODES["TFA_ERR_SHAPE"]
    pv = varlen_params()
    pv.flags = _lib.TFA_FWD_EXACT_MAX
    assert L.tfa_fwd_varlen_local_variant(C.byref(pv), 256, 0) == CODES["TFA_ERR_SHAPE"]


def test_refusal_per_tile_descriptors():
    """A slice that needs per-tile descriptors (the windowed instantiations) has no local form: TFA_ERR_STRIDE."""
    L = _lib.lib()
    N, D = 16384, 128
    p = fwd_params(B=1, H=1, Nq=N, Nk=N, D=D)
    assert plan(p, 256, 0)[0] == 0                                  # the same problem with dense rows runs
    for name in ("q_stride", "k_stride", "v_stride", "o_stride"):
        arr = getattr(p, name)
        arr[2] = 64 * 1024          # rows 128 KiB apart: a 16384-row slice spans 2 GiB
        arr[1] = N * arr[2]
        arr[0] = arr[1]
    assert L.tfa_fwd_plan(C.byref(p), None, None, None) == 0          # tfa_fwd runs it (windowed instantiation)
    assert plan(p, 256, 0)[0] == CODES["TFA_ERR_STRIDE"]
    b = bwd_params(B=1, H=1, Nq=N, Nk=N, D=D)
    assert L.tfa_bwd_local_plan(C.byref(b), 256, 0) == 0
    for name in ("q_stride", "k_stride", "v_stride", "o_stride", "do_stride", "dq_stride", "dk_stride", "dv_stride"):
        arr = getattr(b, name)
        arr[2] = 64 * 1024
        arr[1] = N * arr[2]
        arr[0] = arr[1]
    assert L.tfa_bwd_local_plan(C.byref(b), 256, 0) == CODES["TFA_ERR_STRIDE"]


def test_python_rejections():
    q = torch.zeros(1, 128, 2, 64, dtype=torch.float32)
    with pytest.raises(ValueError, match="float16 / bfloat16"):
        ops._window((64, 0), False, 128, 128, torch.float32, 64)
    with pytest.raises(ValueError, match="up to 128"):
        ops._window((64, 0), False, 128, 128, torch.bfloat16, 256)
    with pytest.raises(ValueError, match=">= -1"):
        ops._window((-2, 0), False, 128, 128, torch.bfloat16, 64)
    with pytest.raises(ValueError, match="pair"):
        ops._window(64, False, 128, 128, torch.bfloat16, 64)
    with pytest.raises(ValueError, match="exact_max"):
        ops._window((64, 0), False, 128, 128, torch.bfloat16, 64, extra=((True, "no exact_max form"),))
    # normalisation: full / causal windows run the existing entry points
    assert ops._window((-1, -1), False, 128, 128, torch.float32, 256) is None
    assert ops._window((-1, -1), True, 128, 128, torch.float32, 256) is None
    assert ops._window((-1, 0), False, 128, 128, torch.bfloat16, 64) == (-1, 0)
    assert ops._window((500, 7), True, 128, 128, torch.bfloat16, 64) is None       # left reaches every key, causal: plain causal
    assert ops._window((64, 300), False, 128, 128, torch.bfloat16, 64) == (64, -1)
    assert ops._window((64, 3), True, 128, 128, torch.bfloat16, 64) == (64, 0)
    del q
