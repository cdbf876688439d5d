"""CPU tests of the ALiBi entry points (include/tfa.h: tfa_fwd_alibi, tfa_bwd_alibi, their varlen forms and the _plan / _variant / _rounding_rule
companions): symbols, plans, kernel choice, rounding rule, refusal codes, and the Python helper's / wrappers' host-side behaviour.  No GPU: plans
never launch, refused calls return before any launch, the slopes are never read on the host (a stand-in address serves), and the Python helper
refuses before it touches a device."""
import ctypes as C
import inspect

import pytest
import torch

from tiny_flash_attention_amd import _lib, ops

ADDR = 0x10000          # a 16-byte aligned stand-in for device pointers (plans never dereference them)
CODES = {"TFA_ERR_NULL": -1, "TFA_ERR_DTYPE": -2, "TFA_ERR_HEAD_DIM": -3, "TFA_ERR_SHAPE": -4, "TFA_ERR_STRIDE": -5, "TFA_ERR_ALIGN": -6,
         "TFA_ERR_VARIANT": -7}
ALIBI_SYMBOLS = ("tfa_fwd_alibi", "tfa_fwd_alibi_plan", "tfa_fwd_alibi_variant", "tfa_fwd_alibi_rounding_rule",
                 "tfa_fwd_varlen_alibi", "tfa_fwd_varlen_alibi_plan", "tfa_fwd_varlen_alibi_variant", "tfa_fwd_varlen_alibi_rounding_rule",
                 "tfa_bwd_alibi", "tfa_bwd_alibi_plan", "tfa_bwd_varlen_alibi", "tfa_bwd_varlen_alibi_plan")
WINDOWS = [(-1, -1), (-1, 0), (256, 0), (128, 128), (-1, 64), (64, -1)]


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


def varlen_bwd_params(B=4, H=8, Hk=8, D=128, max_q=1024, max_k=1024, total_q=4096, total_k=4096, causal=False, dtype=_lib.TFA_BF16):
    p = _lib.TfaVarlenBwdParams()
    for f in ("q", "k", "v", "out", "dout", "lse", "dq", "dk", "dv", "delta", "cu_seqlens_q", "cu_seqlens_k"):
        setattr(p, f, ADDR)
    p.B, p.H, p.Hk, p.D = B, H, Hk, D
    p.max_seqlen_q, p.max_seqlen_k, p.total_q, p.total_k = max_q, max_k, total_q, total_k
    for name, heads in (("q_stride", H), ("k_stride", Hk), ("v_stride", Hk), ("o_stride", H), ("do_stride", H),
                        ("dq_stride", H), ("dk_stride", Hk), ("dv_stride", Hk)):
        arr = getattr(p, name)
        arr[0], arr[1] = D, heads * D
    p.softmax_scale = 0.125
    p.is_causal = 1 if causal else 0
    p.dtype = p.grad_dtype = dtype
    return p


def plan(p, window, slopes=ADDR, bs=0, varlen=False):
    g, b, l = C.c_int(), C.c_int(), C.c_int()
    f = _lib.lib().tfa_fwd_varlen_alibi_plan if varlen else _lib.lib().tfa_fwd_alibi_plan
    return f(C.byref(p), slopes, bs, window[0], window[1], C.byref(g), C.byref(b), C.byref(l)), g.value, b.value


def every_entry(slopes, bs, window, fkw=None, vkw=None):
    """The status of every dry entry point for one set of slope arguments: forward / backward, fixed-length / varlen."""
    L = _lib.lib()
    fkw, vkw = fkw or {}, vkw or {}
    bkw = {k: v for k, v in fkw.items() if k != "out_dtype"}
    pf, pv, pb, pvb = fwd_params(**fkw), varlen_params(**vkw), bwd_params(**bkw), varlen_bwd_params(**vkw)
    if "out_dtype" in fkw:
        pv.out_dtype = fkw["out_dtype"]
    return {
        "fwd_plan": plan(pf, window, slopes, bs)[0],
        "fwd_variant": L.tfa_fwd_alibi_variant(C.byref(pf), slopes, bs, *window),
        "fwd_rule": L.tfa_fwd_alibi_rounding_rule(C.byref(pf), slopes, bs, *window),
        "varlen_plan": plan(pv, window, slopes, bs, varlen=True)[0],
        "varlen_variant": L.tfa_fwd_varlen_alibi_variant(C.byref(pv), slopes, bs, *window),
        "varlen_rule": L.tfa_fwd_varlen_alibi_rounding_rule(C.byref(pv), slopes, bs, *window),
        "bwd_plan": L.tfa_bwd_alibi_plan(C.byref(pb), slopes, bs, *window),
        "varlen_bwd_plan": L.tfa_bwd_varlen_alibi_plan(C.byref(pvb), slopes, bs, *window),
    }


def test_symbols_exported():
    L = _lib.lib()
    for s in ALIBI_SYMBOLS:
        assert s in _lib.SYMBOLS
        getattr(L, s)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("B,H", [(2, 8), (8, 32)])
def test_plan_variant_rule(window, causal, B, H):
    """Every window — full and causal included — is accepted and runs the local form's kernels: variant 30 / 32, one query block per work item,
    TFA_RULE_LAZY; shared (stride 0) and per-batch (stride H) slopes."""
    L = _lib.lib()
    for bs in (0, H):
        p = fwd_params(B=B, H=H, causal=causal)
        st, grid, block = plan(p, window, bs=bs)
        assert st == 0
        v = L.tfa_fwd_alibi_variant(C.byref(p), ADDR, bs, *window)
        assert v in (30, 32)
        assert v == L.tfa_fwd_local_variant(C.byref(fwd_params(B=B, H=H)), 256, 0)       # as the local form chooses
        bm, wg = (256, 512) if v == 30 else (128, 256)
        assert block == wg and grid == B * H * ((1024 + bm - 1) // bm)                    # no causal pairs
        assert L.tfa_fwd_alibi_rounding_rule(C.byref(p), ADDR, bs, *window) == _lib.RULE_LAZY
        pv = varlen_params(B=B, H=H, Hk=H, causal=causal)
        assert plan(pv, window, bs=bs, varlen=True)[0] == 0
        assert L.tfa_fwd_varlen_alibi_variant(C.byref(pv), ADDR, bs, *window) in (30, 32)
        assert L.tfa_fwd_varlen_alibi_rounding_rule(C.byref(pv), ADDR, bs, *window) == _lib.RULE_LAZY
        assert L.tfa_bwd_alibi_plan(C.byref(bwd_params(B=B, H=H, causal=causal)), ADDR, bs, *window) == 0
        assert L.tfa_bwd_varlen_alibi_plan(C.byref(varlen_bwd_params(B=B, H=H, Hk=H, causal=causal)), ADDR, bs, *window) == 0


@pytest.mark.parametrize("dtype", [_lib.TFA_BF16, _lib.TFA_F16])
@pytest.mark.parametrize("D", [40, 64, 96, 128])
def test_rounding_rule_is_lazy_for_both_dtypes(dtype, D):
    L = _lib.lib()
    for window in ((-1, -1), (-1, 0), (100, 0)):
        assert L.tfa_fwd_alibi_rounding_rule(C.byref(fwd_params(D=D, dtype=dtype)), ADDR, 0, *window) == _lib.RULE_LAZY
        assert L.tfa_fwd_varlen_alibi_rounding_rule(C.byref(varlen_params(D=D, dtype=dtype)), ADDR, 0, *window) == _lib.RULE_LAZY


def test_forced_variant():
    L = _lib.lib()
    try:
        for v in (30, 32):
            _lib.set_variant(v)
            for window in ((-1, -1), (-1, 0), (256, 0)):
                assert L.tfa_fwd_alibi_variant(C.byref(fwd_params()), ADDR, 0, *window) == v
                assert L.tfa_fwd_varlen_alibi_variant(C.byref(varlen_params()), ADDR, 0, *window) == v
        _lib.set_variant(17)
        for window in ((-1, -1), (256, 0)):
            assert L.tfa_fwd_alibi_variant(C.byref(fwd_params()), ADDR, 0, *window) == CODES["TFA_ERR_VARIANT"]
            assert plan(fwd_params(), window)[0] == CODES["TFA_ERR_VARIANT"]
            assert L.tfa_fwd_varlen_alibi_variant(C.byref(varlen_params()), ADDR, 0, *window) == CODES["TFA_ERR_VARIANT"]
            assert L.tfa_fwd_alibi(C.byref(fwd_params()), ADDR, 0, window[0], window[1], None) == CODES["TFA_ERR_VARIANT"]
    finally:
        _lib.set_variant(-1)


@pytest.mark.parametrize("window", [(-1, -1), (-1, 0), (256, 0)])
@pytest.mark.parametrize("slopes,bs,code", [
    (None, 0, "TFA_ERR_NULL"), (ADDR + 2, 0, "TFA_ERR_ALIGN"), (ADDR + 1, 8, "TFA_ERR_ALIGN"),
    (ADDR, 1, "TFA_ERR_STRIDE"), (ADDR, 7, "TFA_ERR_STRIDE"), (ADDR, 16, "TFA_ERR_STRIDE"), (ADDR, -8, "TFA_ERR_STRIDE"),
])
def test_slope_argument_refusals(window, slopes, bs, code):
    """NULL, misaligned slopes and a batch stride other than 0 or H (H = 8 here): every entry point, fixed-length and varlen, forward and backward."""
    L = _lib.lib()
    want = CODES[code]
    assert set(every_entry(slopes, bs, window).values()) == {want}
    # the launching entry points refuse before any launch
    assert L.tfa_fwd_alibi(C.byref(fwd_params()), slopes, bs, window[0], window[1], None) == want
    assert L.tfa_fwd_varlen_alibi(C.byref(varlen_params()), slopes, bs, window[0], window[1], None) == want
    assert L.tfa_bwd_alibi(C.byref(bwd_params()), slopes, bs, window[0], window[1], None) == want
    assert L.tfa_bwd_varlen_alibi(C.byref(varlen_bwd_params()), slopes, bs, window[0], window[1], None) == want


def test_four_byte_aligned_slopes_accepted():
    st = every_entry(ADDR + 4, 8, (-1, 0))
    assert st["fwd_plan"] == st["varlen_plan"] == st["bwd_plan"] == st["varlen_bwd_plan"] == 0
    assert st["fwd_variant"] in (30, 32) and st["varlen_variant"] in (30, 32)
    assert st["fwd_rule"] == st["varlen_rule"] == _lib.RULE_LAZY


@pytest.mark.parametrize("window", [(-1, -1), (-1, 0), (256, 0)])
@pytest.mark.parametrize("kw,code", [
    (dict(D=136), "TFA_ERR_HEAD_DIM"), (dict(D=256), "TFA_ERR_HEAD_DIM"),
    (dict(dtype=_lib.TFA_F32, out_dtype=_lib.TFA_F32), "TFA_ERR_DTYPE"),
])
def test_local_form_refusals(window, kw, code):
    """What the local form refuses, with its codes — also for the full and causal masks, which without slopes would run tfa_fwd's kernels."""
    vkw = {k: v for k, v in kw.items() if k in ("D", "dtype")}
    assert set(every_entry(ADDR, 0, window, fkw=kw, vkw=vkw).values()) == {CODES[code]}


@pytest.mark.parametrize("window", [(-2, 0), (0, -2), (-5, -5)])
def test_window_side_below_minus_one(window):
    assert set(every_entry(ADDR, 0, window).values()) == {CODES["TFA_ERR_SHAPE"]}


def test_refusal_flags_and_partial_passes():
    L = _lib.lib()
    for window in ((-1, -1), (-1, 0), (256, 0)):
        p = fwd_params()
        p.flags = _lib.TFA_FWD_EXACT_MAX
        assert plan(p, window)[0] == CODES["TFA_ERR_SHAPE"]
        assert L.tfa_fwd_alibi_variant(C.byref(p), ADDR, 0, *window) == CODES["TFA_ERR_SHAPE"]
        p.flags = 0
        p.kv_offset = 64
        assert plan(p, window)[0] == CODES["TFA_ERR_SHAPE"]
        p.kv_offset = 0
        p.nk_total = 2048
        assert plan(p, window)[0] == CODES["TFA_ERR_SHAPE"]
        pv = varlen_params()
        pv.flags = _lib.TFA_FWD_EXACT_MAX
        assert L.tfa_fwd_varlen_alibi_variant(C.byref(pv), ADDR, 0, *window) == CODES["TFA_ERR_SHAPE"]
        pvb = varlen_bwd_params()
        pvb.flags = 1
        assert L.tfa_bwd_varlen_alibi_plan(C.byref(pvb), ADDR, 0, *window) == CODES["TFA_ERR_SHAPE"]


def test_refusal_long_sequences():
    """Nq + Nk >= 2^28: the kernels' distance / window arithmetic is int32 with room to spare."""
    L = _lib.lib()
    N = 1 << 27
    for window in ((-1, -1), (-1, 0)):
        assert plan(fwd_params(B=1, H=1, Nq=N, Nk=N, D=64), window)[0] == CODES["TFA_ERR_SHAPE"]
        assert L.tfa_bwd_alibi_plan(C.byref(bwd_params(B=1, H=1, Nq=N, Nk=N, D=64)), ADDR, 0, *window) == CODES["TFA_ERR_SHAPE"]
        assert plan(varlen_params(B=1, H=1, Hk=1, D=64, max_q=N, max_k=N, total_q=N, total_k=N), window, varlen=True)[0] == CODES["TFA_ERR_SHAPE"]
        pvb = varlen_bwd_params(B=1, H=1, Hk=1, D=64, max_q=N, max_k=N, total_q=N, total_k=N)
        assert L.tfa_bwd_varlen_alibi_plan(C.byref(pvb), ADDR, 0, *window) == CODES["TFA_ERR_SHAPE"]


def test_refusal_per_tile_descriptors():
    """A slice that needs per-tile descriptors has no local form and so no ALiBi form: TFA_ERR_STRIDE, also for the plain causal mask."""
    L = _lib.lib()
    N, D = 16384, 128
    for window in ((-1, 0), (256, 0)):
        p = fwd_params(B=1, H=1, Nq=N, Nk=N, D=D)
        assert plan(p, window)[0] == 0                                # the same problem with dense rows runs
        for name in ("q_stride", "k_stride", "v_stride", "o_stride"):
            arr = getattr(p, name)
            arr[2] = 64 * 1024          # rows 128 KiB apart: a 16384-row slice spans 2 GiB
            arr[1] = N * arr[2]
            arr[0] = arr[1]
        assert L.tfa_fwd_plan(C.byref(p), None, None, None) == 0      # tfa_fwd runs it (windowed instantiation)
        assert plan(p, window)[0] == CODES["TFA_ERR_STRIDE"]
        b = bwd_params(B=1, H=1, Nq=N, Nk=N, D=D)
        assert L.tfa_bwd_alibi_plan(C.byref(b), ADDR, 0, *window) == 0
        for name in ("q_stride", "k_stride", "v_stride", "o_stride", "do_stride", "dq_stride", "dk_stride", "dv_stride"):
            arr = getattr(b, name)
            arr[2] = 64 * 1024
            arr[1] = N * arr[2]
            arr[0] = arr[1]
        assert L.tfa_bwd_alibi_plan(C.byref(b), ADDR, 0, *window) == CODES["TFA_ERR_STRIDE"]


def test_null_params():
    L = _lib.lib()
    assert L.tfa_fwd_alibi_plan(None, ADDR, 0, -1, -1, None, None, None) == CODES["TFA_ERR_NULL"]
    assert L.tfa_fwd_varlen_alibi_variant(None, ADDR, 0, -1, -1) == CODES["TFA_ERR_NULL"]
    assert L.tfa_bwd_alibi_plan(None, ADDR, 0, -1, -1) == CODES["TFA_ERR_NULL"]
    assert L.tfa_bwd_varlen_alibi_plan(None, ADDR, 0, -1, -1) == CODES["TFA_ERR_NULL"]


def test_existing_entry_points_keep_their_rule():
    """Without slopes the existing entry points plan what they planned (bf16: the first-tile rule); with slopes the same problem is TFA_RULE_LAZY."""
    L = _lib.lib()
    p = fwd_params(B=8, H=32, Nq=4096, Nk=4096, causal=True)
    assert L.tfa_fwd_variant(C.byref(p)) == 30 and L.tfa_fwd_rounding_rule(C.byref(p)) == _lib.RULE_FIRST_TILE
    assert L.tfa_fwd_local_rounding_rule(C.byref(p), -1, 0) == _lib.RULE_FIRST_TILE
    assert L.tfa_fwd_alibi_rounding_rule(C.byref(p), ADDR, 0, -1, 0) == _lib.RULE_LAZY


# ---- Python: the helper and the wrappers' keyword plumbing ------------------------------------------------------------------------------
def test_python_helper_accepts():
    cpu = torch.device("cpu")
    assert ops._alibi(None, 2, 8, cpu, torch.float32, 256) is None                       # no slopes: nothing is checked, the existing calls run
    s1 = torch.zeros(8, dtype=torch.float32)
    s2 = torch.zeros(2, 8, dtype=torch.float32)
    t, bs = ops._alibi(s1, 2, 8, cpu, torch.bfloat16, 128)
    assert t is s1 and bs == 0
    t, bs = ops._alibi(s2, 2, 8, cpu, torch.float16, 40)
    assert t is s2 and bs == 8
    assert ops._alibi(torch.zeros(1, 8), 1, 8, cpu, torch.bfloat16, 64)[1] == 8          # (B, H) with B = 1 is still per-batch
    s1.requires_grad_(True)
    assert ops._alibi(s1, 2, 8, cpu, torch.bfloat16, 64)[0] is s1                        # may require grad; it just gets none
    assert ops._alibi_window(None, False) == (-1, -1) and ops._alibi_window(None, True) == (-1, 0) and ops._alibi_window((64, 0), True) == (64, 0)


def test_python_helper_rejections():
    cpu = torch.device("cpu")
    ok = torch.zeros(2, 8, dtype=torch.float32)
    for bad in (torch.zeros(8, dtype=torch.float64), torch.zeros(8, dtype=torch.bfloat16), torch.zeros(8, dtype=torch.int32), [0.5] * 8):
        with pytest.raises(TypeError, match="float32"):
            ops._alibi(bad, 2, 8, cpu, torch.bfloat16, 64)
    for shape in ((4,), (8, 2), (3, 8), (2, 8, 1), (1, 8), ()):
        with pytest.raises(ValueError, match="shape"):
            ops._alibi(torch.zeros(shape, dtype=torch.float32), 2, 8, cpu, torch.bfloat16, 64)
    with pytest.raises(ValueError, match="contiguous"):
        ops._alibi(torch.zeros(8, 2, dtype=torch.float32).t(), 2, 8, cpu, torch.bfloat16, 64)
    with pytest.raises(ValueError, match="contiguous"):
        ops._alibi(torch.zeros(16, dtype=torch.float32)[::2], 2, 8, cpu, torch.bfloat16, 64)
    with pytest.raises(ValueError, match="device"):
        ops._alibi(ok, 2, 8, torch.device("meta"), torch.bfloat16, 64)
    with pytest.raises(ValueError, match="float16 / bfloat16"):
        ops._alibi(ok, 2, 8, cpu, torch.float32, 64)
    with pytest.raises(ValueError, match="up to 128"):
        ops._alibi(ok, 2, 8, cpu, torch.bfloat16, 136)
    with pytest.raises(ValueError, match="exact_max"):
        ops._alibi(ok, 2, 8, cpu, torch.bfloat16, 64, extra=((True, "no exact_max form of the ALiBi kernels"),))
    with pytest.raises(ValueError, match="split-KV"):
        ops._alibi(ok, 2, 8, cpu, torch.bfloat16, 64, extra=((False, "x"), (True, "no split-KV / partial passes")))


def test_wrappers_take_alibi_slopes_as_last_keyword():
    import tiny_flash_attention_amd as tfa

    for f in (tfa.flash_attn_func, tfa.flash_attn_varlen_func, ops.flash_attn_fwd, ops.flash_attn_bwd, ops.flash_attn_varlen_fwd, ops.flash_attn_varlen_bwd):
        params = list(inspect.signature(f).parameters.values())
        assert params[-1].name == "alibi_slopes" and params[-1].default is None, f.__name__
    for cls in (ops._FlashAttnBNHD, ops._FlashAttnVarlen):
        params = list(inspect.signature(cls.forward).parameters.values())
        assert params[-1].name == "alibi_slopes" and params[-1].default is None


def test_varlen_func_still_refuses_dropout():
    import tiny_flash_attention_amd as tfa

    x = torch.zeros(4, 2, 64, dtype=torch.bfloat16)
    cu = torch.tensor([0, 4], dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="dropout"):
        tfa.flash_attn_varlen_func(x, x, x, cu, cu, 4, 4, dropout_p=0.1, alibi_slopes=torch.zeros(2, dtype=torch.float32))
