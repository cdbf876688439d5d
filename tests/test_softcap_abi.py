"""CPU tests of the soft-capping entry points (include/tfa.h: tfa_fwd_softcap, tfa_bwd_softcap, their varlen forms and the _plan / _variant /
_rounding_rule companions): symbols, plans, kernel choice, rounding rule, refusal codes, and the Python checker's / wrappers' host-side behaviour.  No
GPU: plans never launch, refused calls return before any launch, the slopes are never read on the host (a stand-in address serves), softcap is a host
float, and the Python checker refuses before it touches a device."""
import ctypes as C
import inspect
import math

import pytest
import torch

from tiny_flash_attention_amd import _lib, ops

ADDR = 0x10000          # a 16-byte aligned stand-in for device pointers (plans never dereference them)
CODES = {"TFA_ERR_NULL": -1, "TFA_ERR_DTYPE": -2, "TFA_ERR_HEAD_DIM": -3, "TFA_ERR_SHAPE": -4, "TFA_ERR_STRIDE": -5, "TFA_ERR_ALIGN": -6,
         "TFA_ERR_VARIANT": -7, "TFA_ERR_SCALE": -8}
SOFTCAP_SYMBOLS = ("tfa_fwd_softcap", "tfa_fwd_softcap_plan", "tfa_fwd_softcap_variant", "tfa_fwd_softcap_rounding_rule",
                   "tfa_fwd_varlen_softcap", "tfa_fwd_varlen_softcap_plan", "tfa_fwd_varlen_softcap_variant", "tfa_fwd_varlen_softcap_rounding_rule",
                   "tfa_bwd_softcap", "tfa_bwd_softcap_plan", "tfa_bwd_varlen_softcap", "tfa_bwd_varlen_softcap_plan")
WINDOWS = [(-1, -1), (-1, 0), (256, 0), (128, 128), (-1, 64), (64, -1)]
CAP = 50.0


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


def plan(p, window, cap=CAP, slopes=None, bs=0, varlen=False):
    g, b, l = C.c_int(), C.c_int(), C.c_int()
    f = _lib.lib().tfa_fwd_varlen_softcap_plan if varlen else _lib.lib().tfa_fwd_softcap_plan
    return f(C.byref(p), cap, slopes, bs, window[0], window[1], C.byref(g), C.byref(b), C.byref(l)), g.value, b.value, l.value


def alibi_plan(p, window, bs=0, varlen=False):
    g, b, l = C.c_int(), C.c_int(), C.c_int()
    f = _lib.lib().tfa_fwd_varlen_alibi_plan if varlen else _lib.lib().tfa_fwd_alibi_plan
    return f(C.byref(p), ADDR, bs, window[0], window[1], C.byref(g), C.byref(b), C.byref(l)), g.value, b.value, l.value


def every_entry(cap, slopes, bs, window, fkw=None, vkw=None):
    """The status of every dry entry point for one set of cap / slope arguments: forward / backward, fixed-length / varlen."""
    L = _lib.lib()
    fkw, vkw = fkw or {}, vkw or {}
    bkw = {k: v for k, v in fkw.items() if k != "out_dtype"}
    pf, pv, pb, pvb = fwd_params(**fkw), varlen_params(**vkw), bwd_params(**bkw), varlen_bwd_params(**vkw)
    if "out_dtype" in fkw:
        pv.out_dtype = fkw["out_dtype"]
    return {
        "fwd_plan": plan(pf, window, cap, slopes, bs)[0],
        "fwd_variant": L.tfa_fwd_softcap_variant(C.byref(pf), cap, slopes, bs, *window),
        "fwd_rule": L.tfa_fwd_softcap_rounding_rule(C.byref(pf), cap, slopes, bs, *window),
        "varlen_plan": plan(pv, window, cap, slopes, bs, varlen=True)[0],
        "varlen_variant": L.tfa_fwd_varlen_softcap_variant(C.byref(pv), cap, slopes, bs, *window),
        "varlen_rule": L.tfa_fwd_varlen_softcap_rounding_rule(C.byref(pv), cap, slopes, bs, *window),
        "bwd_plan": L.tfa_bwd_softcap_plan(C.byref(pb), cap, slopes, bs, *window),
        "varlen_bwd_plan": L.tfa_bwd_varlen_softcap_plan(C.byref(pvb), cap, slopes, bs, *window),
    }


def launching_entries(cap, slopes, bs, window):
    """The status of the four launching entry points (they must refuse before any launch: there is no GPU here)."""
    L = _lib.lib()
    return {L.tfa_fwd_softcap(C.byref(fwd_params()), cap, slopes, bs, window[0], window[1], None),
            L.tfa_fwd_varlen_softcap(C.byref(varlen_params()), cap, slopes, bs, window[0], window[1], None),
            L.tfa_bwd_softcap(C.byref(bwd_params()), cap, slopes, bs, window[0], window[1], None),
            L.tfa_bwd_varlen_softcap(C.byref(varlen_bwd_params()), cap, slopes, bs, window[0], window[1], None)}


def test_symbols_exported_and_version():
    L = _lib.lib()
    for s in SOFTCAP_SYMBOLS:
        assert s in _lib.SYMBOLS
        getattr(L, s)
    assert L.tfa_version() == 111


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("B,H", [(2, 8), (8, 32)])
def test_plan_variant_rule_agree_with_the_alibi_form(window, causal, B, H):
    """Every window — full and causal included — with and without slopes plans what the ALiBi form plans for the same problem: variant 30 / 32, one query
    block per work item, the same grid, block and LDS, TFA_RULE_LAZY; fixed-length and varlen, forward and backward."""
    L = _lib.lib()
    for slopes, bs in ((None, 0), (ADDR, 0), (ADDR, H)):
        p = fwd_params(B=B, H=H, causal=causal)
        st, grid, block, lds = plan(p, window, CAP, slopes, bs)
        assert st == 0
        assert (st, grid, block, lds) == alibi_plan(p, window, bs if slopes else 0)
        v = L.tfa_fwd_softcap_variant(C.byref(p), CAP, slopes, bs, *window)
        assert v in (30, 32) and v == L.tfa_fwd_alibi_variant(C.byref(p), ADDR, 0, *window)
        bm, wg = (256, 512) if v == 30 else (128, 256)
        assert block == wg and grid == B * H * ((1024 + bm - 1) // bm)                    # no causal pairs
        assert L.tfa_fwd_softcap_rounding_rule(C.byref(p), CAP, slopes, bs, *window) == _lib.RULE_LAZY
        pv = varlen_params(B=B, H=H, Hk=H, causal=causal)
        assert plan(pv, window, CAP, slopes, bs, varlen=True) == alibi_plan(pv, window, bs if slopes else 0, varlen=True)
        assert plan(pv, window, CAP, slopes, bs, varlen=True)[0] == 0
        assert L.tfa_fwd_varlen_softcap_variant(C.byref(pv), CAP, slopes, bs, *window) == L.tfa_fwd_varlen_alibi_variant(C.byref(pv), ADDR, 0, *window)
        assert L.tfa_fwd_varlen_softcap_rounding_rule(C.byref(pv), CAP, slopes, bs, *window) == _lib.RULE_LAZY
        assert L.tfa_bwd_softcap_plan(C.byref(bwd_params(B=B, H=H, causal=causal)), CAP, slopes, bs, *window) == 0
        assert L.tfa_bwd_varlen_softcap_plan(C.byref(varlen_bwd_params(B=B, H=H, Hk=H, causal=causal)), CAP, slopes, bs, *window) == 0


@pytest.mark.parametrize("dtype", [_lib.TFA_BF16, _lib.TFA_F16])
@pytest.mark.parametrize("D", [40, 64, 96, 128])
def test_rounding_rule_is_lazy_for_both_dtypes(dtype, D):
    L = _lib.lib()
    for window in ((-1, -1), (-1, 0), (100, 0)):
        for slopes in (None, ADDR):
            assert L.tfa_fwd_softcap_rounding_rule(C.byref(fwd_params(D=D, dtype=dtype)), CAP, slopes, 0, *window) == _lib.RULE_LAZY
            assert L.tfa_fwd_varlen_softcap_rounding_rule(C.byref(varlen_params(D=D, dtype=dtype)), CAP, slopes, 0, *window) == _lib.RULE_LAZY


@pytest.mark.parametrize("cap", [1e-3, 1.0, 30.0, 50.0, 1e6])
def test_any_positive_finite_cap_plans(cap):
    st = every_entry(cap, None, 0, (-1, 0))
    assert st["fwd_plan"] == st["varlen_plan"] == st["bwd_plan"] == st["varlen_bwd_plan"] == 0
    assert st["fwd_rule"] == st["varlen_rule"] == _lib.RULE_LAZY


def test_forced_variant():
    L = _lib.lib()
    try:
        for v in (30, 32):
            _lib.set_variant(v)
            for window in ((-1, -1), (-1, 0), (256, 0)):
                assert L.tfa_fwd_softcap_variant(C.byref(fwd_params()), CAP, None, 0, *window) == v
                assert L.tfa_fwd_varlen_softcap_variant(C.byref(varlen_params()), CAP, ADDR, 0, *window) == v
        _lib.set_variant(17)                                                              # a foreign variant
        for window in ((-1, -1), (256, 0)):
            assert L.tfa_fwd_softcap_variant(C.byref(fwd_params()), CAP, None, 0, *window) == CODES["TFA_ERR_VARIANT"]
            assert plan(fwd_params(), window)[0] == CODES["TFA_ERR_VARIANT"]
            assert L.tfa_fwd_varlen_softcap_variant(C.byref(varlen_params()), CAP, None, 0, *window) == CODES["TFA_ERR_VARIANT"]
            assert L.tfa_fwd_softcap(C.byref(fwd_params()), CAP, None, 0, window[0], window[1], None) == CODES["TFA_ERR_VARIANT"]
    finally:
        _lib.set_variant(-1)


@pytest.mark.parametrize("window", [(-1, -1), (-1, 0), (256, 0)])
@pytest.mark.parametrize("cap", [0.0, -0.0, -1.0, -50.0, float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("slopes", [None, ADDR])
def test_bad_softcap_is_refused_at_the_c_boundary(window, cap, slopes):
    """softcap <= 0 (0 included: a C caller without a cap uses the other entry points), NaN and +-inf: TFA_ERR_SCALE from every entry point, nothing launched."""
    want = CODES["TFA_ERR_SCALE"]
    assert set(every_entry(cap, slopes, 0, window).values()) == {want}
    assert launching_entries(cap, slopes, 0, window) == {want}


def test_cap_beyond_fp32_over_the_scale_is_refused():
    """The kernels work with softcap / softmax_scale: a cap that leaves fp32 there is refused, not turned into inf."""
    L = _lib.lib()
    p = fwd_params()
    p.softmax_scale = 1e-30
    assert L.tfa_fwd_softcap_variant(C.byref(p), 1e30, None, 0, -1, -1) == CODES["TFA_ERR_SCALE"]
    assert L.tfa_fwd_softcap_variant(C.byref(p), 1.0, None, 0, -1, -1) in (30, 32)


@pytest.mark.parametrize("window", [(-1, -1), (-1, 0), (256, 0)])
@pytest.mark.parametrize("slopes,bs,code", [
    (ADDR + 2, 0, "TFA_ERR_ALIGN"), (ADDR + 1, 8, "TFA_ERR_ALIGN"),
    (ADDR, 1, "TFA_ERR_STRIDE"), (ADDR, 7, "TFA_ERR_STRIDE"), (ADDR, 16, "TFA_ERR_STRIDE"), (ADDR, -8, "TFA_ERR_STRIDE"),
])
def test_bad_slopes_are_refused(window, slopes, bs, code):
    """With slopes, what the ALiBi entry points refuse for them (H = 8 here); NULL slopes are legal here and mean "no bias"."""
    want = CODES[code]
    assert set(every_entry(CAP, slopes, bs, window).values()) == {want}
    assert launching_entries(CAP, slopes, bs, window) == {want}
    ok = every_entry(CAP, None, bs, window)                                               # NULL slopes: the stride is not looked at
    assert ok["fwd_plan"] == ok["varlen_plan"] == ok["bwd_plan"] == ok["varlen_bwd_plan"] == 0


@pytest.mark.parametrize("window", [(-1, -1), (-1, 0), (256, 0)])
@pytest.mark.parametrize("slopes", [None, ADDR])
@pytest.mark.parametrize("kw,code", [
    (dict(D=136), "TFA_ERR_HEAD_DIM"), (dict(D=256), "TFA_ERR_HEAD_DIM"),
    (dict(dtype=_lib.TFA_F32, out_dtype=_lib.TFA_F32), "TFA_ERR_DTYPE"),
])
def test_local_form_refusals(window, slopes, kw, code):
    """What the local form refuses, with its codes — also for the full and causal masks, which without a cap would run tfa_fwd's kernels."""
    vkw = {k: v for k, v in kw.items() if k in ("D", "dtype")}
    assert set(every_entry(CAP, slopes, 0, window, fkw=kw, vkw=vkw).values()) == {CODES[code]}


@pytest.mark.parametrize("window", [(-2, 0), (0, -2), (-5, -5)])
def test_window_side_below_minus_one(window):
    assert set(every_entry(CAP, None, 0, window).values()) == {CODES["TFA_ERR_SHAPE"]}


def test_refusal_flags_and_partial_passes():
    L = _lib.lib()
    for window in ((-1, -1), (-1, 0), (256, 0)):
        p = fwd_params()
        p.flags = _lib.TFA_FWD_EXACT_MAX
        assert plan(p, window)[0] == CODES["TFA_ERR_SHAPE"]
        assert L.tfa_fwd_softcap_variant(C.byref(p), CAP, None, 0, *window) == CODES["TFA_ERR_SHAPE"]
        assert L.tfa_fwd_softcap(C.byref(p), CAP, None, 0, window[0], window[1], None) == CODES["TFA_ERR_SHAPE"]
        p.flags = 0
        p.kv_offset = 64
        assert plan(p, window)[0] == CODES["TFA_ERR_SHAPE"]
        p.kv_offset = 0
        p.nk_total = 2048
        assert plan(p, window)[0] == CODES["TFA_ERR_SHAPE"]
        pv = varlen_params()
        pv.flags = _lib.TFA_FWD_EXACT_MAX
        assert L.tfa_fwd_varlen_softcap_variant(C.byref(pv), CAP, None, 0, *window) == CODES["TFA_ERR_SHAPE"]
        pvb = varlen_bwd_params()
        pvb.flags = 1
        assert L.tfa_bwd_varlen_softcap_plan(C.byref(pvb), CAP, None, 0, *window) == CODES["TFA_ERR_SHAPE"]


def test_refusal_long_sequences():
    L = _lib.lib()
    N = 1 << 27
    for window in ((-1, -1), (-1, 0)):
        assert plan(fwd_params(B=1, H=1, Nq=N, Nk=N, D=64), window)[0] == CODES["TFA_ERR_SHAPE"]
        assert L.tfa_bwd_softcap_plan(C.byref(bwd_params(B=1, H=1, Nq=N, Nk=N, D=64)), CAP, None, 0, *window) == CODES["TFA_ERR_SHAPE"]
        assert plan(varlen_params(B=1, H=1, Hk=1, D=64, max_q=N, max_k=N, total_q=N, total_k=N), window, varlen=True)[0] == CODES["TFA_ERR_SHAPE"]
        pvb = varlen_bwd_params(B=1, H=1, Hk=1, D=64, max_q=N, max_k=N, total_q=N, total_k=N)
        assert L.tfa_bwd_varlen_softcap_plan(C.byref(pvb), CAP, None, 0, *window) == CODES["TFA_ERR_SHAPE"]


def test_refusal_per_tile_descriptors():
    """A slice that needs per-tile descriptors has no local form and so no soft-capping form: TFA_ERR_STRIDE, also for the plain causal mask."""
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
        assert L.tfa_bwd_softcap_plan(C.byref(b), CAP, None, 0, *window) == 0
        for name in ("q_stride", "k_stride", "v_stride", "o_stride", "do_stride", "dq_stride", "dk_stride", "dv_stride"):
            arr = getattr(b, name)
            arr[2] = 64 * 1024
            arr[1] = N * arr[2]
            arr[0] = arr[1]
        assert L.tfa_bwd_softcap_plan(C.byref(b), CAP, None, 0, *window) == CODES["TFA_ERR_STRIDE"]


def test_null_params():
    L = _lib.lib()
    assert L.tfa_fwd_softcap_plan(None, CAP, None, 0, -1, -1, None, None, None) == CODES["TFA_ERR_NULL"]
    assert L.tfa_fwd_softcap(None, CAP, None, 0, -1, -1, None) == CODES["TFA_ERR_NULL"]
    assert L.tfa_fwd_varlen_softcap_variant(None, CAP, None, 0, -1, -1) == CODES["TFA_ERR_NULL"]
    assert L.tfa_bwd_softcap_plan(None, CAP, None, 0, -1, -1) == CODES["TFA_ERR_NULL"]
    assert L.tfa_bwd_varlen_softcap_plan(None, CAP, None, 0, -1, -1) == CODES["TFA_ERR_NULL"]


def test_existing_entry_points_keep_their_rule():
    """Without a cap the existing entry points plan what they planned (bf16: the first-tile rule); with one the same problem is TFA_RULE_LAZY."""
    L = _lib.lib()
    p = fwd_params(B=8, H=32, Nq=4096, Nk=4096, causal=True)
    assert L.tfa_fwd_variant(C.byref(p)) == 30 and L.tfa_fwd_rounding_rule(C.byref(p)) == _lib.RULE_FIRST_TILE
    assert L.tfa_fwd_local_rounding_rule(C.byref(p), -1, 0) == _lib.RULE_FIRST_TILE
    assert L.tfa_fwd_softcap_rounding_rule(C.byref(p), CAP, None, 0, -1, 0) == _lib.RULE_LAZY


# ---- Python: the checker and the wrappers' keyword plumbing -----------------------------------------------------------------------------
def test_python_checker_accepts():
    assert ops._softcap(0.0, torch.float32, 256) == 0.0                                  # no cap: nothing else is checked, the existing calls run
    assert ops._softcap(0, torch.bfloat16, 64) == 0.0 and ops._softcap(-0.0, torch.bfloat16, 64) == 0.0
    assert ops._softcap(0.0, torch.bfloat16, 64, extra=((True, "never looked at"),)) == 0.0
    assert ops._softcap(50.0, torch.bfloat16, 128) == 50.0
    assert ops._softcap(30, torch.float16, 40) == 30.0 and isinstance(ops._softcap(30, torch.float16, 40), float)
    assert ops._slopes_arg(None) == (None, 0)


def test_python_checker_rejections():
    for bad in (-1.0, -50, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="softcap must be"):
            ops._softcap(bad, torch.bfloat16, 64)
    with pytest.raises(TypeError, match="host number"):
        ops._softcap(torch.tensor(50.0), torch.bfloat16, 64)
    with pytest.raises(ValueError, match="float16 / bfloat16"):
        ops._softcap(50.0, torch.float32, 64)
    with pytest.raises(ValueError, match="up to 128"):
        ops._softcap(50.0, torch.bfloat16, 136)
    with pytest.raises(ValueError, match="exact_max"):
        ops._softcap(50.0, torch.bfloat16, 64, extra=((True, "no exact_max form of the soft-capping kernels"),))
    with pytest.raises(ValueError, match="split-KV"):
        ops._softcap(50.0, torch.bfloat16, 64, extra=((False, "x"), (True, "no split-KV / partial passes")))
    with pytest.raises(ValueError, match="workspace"):
        ops._softcap(50.0, torch.bfloat16, 64, extra=((True, "no dS-workspace form"),))


def test_wrappers_take_softcap_without_moving_any_argument():
    """`softcap` joins every wrapper as a keyword with default 0.0 directly in front of `alibi_slopes`, which stays the last parameter (tests/test_alibi_abi.py
    pins that).  In the explicit ops forms both are keyword-only, so their order carries no meaning; in flash_attn_func / flash_attn_varlen_func `softcap` is
    keyword-only and `alibi_slopes` is still accepted as the positional argument behind `window_size`: no positional call changes meaning."""
    import tiny_flash_attention_amd as tfa

    for f in (tfa.flash_attn_func, tfa.flash_attn_varlen_func, ops.flash_attn_fwd, ops.flash_attn_bwd, ops.flash_attn_varlen_fwd, ops.flash_attn_varlen_bwd):
        params = list(inspect.signature(f).parameters.values())
        assert params[-1].name == "alibi_slopes" and params[-1].default is None, f.__name__
        assert params[-2].name == "softcap" and params[-2].default == 0.0 and params[-2].kind is inspect.Parameter.KEYWORD_ONLY, f.__name__
    for cls in (ops._FlashAttnBNHD, ops._FlashAttnVarlen):
        params = list(inspect.signature(cls.forward).parameters.values())
        assert params[-1].name == "alibi_slopes" and params[-2].name == "softcap" and params[-2].default == 0.0
    for f, n in ((tfa.flash_attn_func, 6), (tfa.flash_attn_varlen_func, 11)):            # the positional parameters are those of the parent interface
        params = list(inspect.signature(f).parameters.values())
        assert params[n - 1].name == "window_size" and params[n].kind is inspect.Parameter.VAR_POSITIONAL
    s = object()
    assert ops._positional_slopes((), None, "f") is None and ops._positional_slopes((s,), None, "f") is s and ops._positional_slopes((), s, "f") is s
    for extra, kw in (((s, 50.0), None), ((s,), s)):
        with pytest.raises(TypeError, match="alibi_slopes"):
            ops._positional_slopes(extra, kw, "f")


class _CountingLib:
    """A stand-in for the loaded library object: counts the calls by entry point and answers TFA_OK, launching nothing."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if name in ("tfa_fwd_suggest_splits",):
            return lambda *a: 1

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
    """A tensor the wrappers accept as a CUDA tensor without a GPU: storage-less, is_cuda patched in by the caller's monkeypatch."""
    return torch.empty(shape, dtype=dtype, device="meta")


@pytest.fixture
def stub(monkeypatch):
    fake = _CountingLib(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    monkeypatch.setattr(ops.torch, "cuda", _FakeCuda)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(torch.Tensor, "data_ptr", lambda self: ADDR)
    return fake


def test_softcap_zero_reaches_the_old_entry_points(stub):
    """softcap=0.0 (and the keyword left out) calls exactly the entry points it called before the argument existed; softcap > 0 the _softcap ones, with the
    cap as a float, NULL for missing slopes, and the window the ALiBi entry points would be given."""
    q, k = _meta(2, 4, 256, 64), _meta(2, 4, 256, 64)
    slopes = _meta(4, dtype=torch.float32)
    names = lambda: [c[0] for c in stub.calls]

    for kw in ({}, {"softcap": 0.0}, {"softcap": 0}):
        stub.calls.clear()
        ops.flash_attn_fwd(q, k, k, True, **kw)
        ops.flash_attn_fwd(q, k, k, False, window_size=(64, 0), **kw)
        ops.flash_attn_fwd(q, k, k, True, alibi_slopes=slopes, **kw)
        assert names() == ["tfa_fwd", "tfa_fwd_local", "tfa_fwd_alibi"], kw

    stub.calls.clear()
    ops.flash_attn_fwd(q, k, k, True, softcap=50.0)
    ops.flash_attn_fwd(q, k, k, False, window_size=(64, 0), softcap=30)
    ops.flash_attn_fwd(q, k, k, False, alibi_slopes=slopes, softcap=5.0)
    assert names() == ["tfa_fwd_softcap"] * 3
    a0, a1, a2 = (c[1] for c in stub.calls)
    assert (a0[1], a0[2], a0[3], a0[4], a0[5]) == (50.0, None, 0, -1, 0)                 # causal: (-1, 0), no slopes: NULL
    assert (a1[1], a1[2], a1[4], a1[5]) == (30.0, None, 64, 0) and isinstance(a1[1], float)
    assert (a2[1], a2[2], a2[3], a2[4], a2[5]) == (5.0, ADDR, 0, -1, -1)

    out, lse = _meta(2, 4, 256, 64), _meta(2, 4, 256, dtype=torch.float32)
    for kw in ({}, {"softcap": 0.0}):
        stub.calls.clear()
        ops.flash_attn_bwd(q, k, k, out, lse, out, True, **kw)
        ops.flash_attn_bwd(q, k, k, out, lse, out, False, window_size=(64, 0), **kw)
        ops.flash_attn_bwd(q, k, k, out, lse, out, True, alibi_slopes=slopes, **kw)
        assert names() == ["tfa_bwd", "tfa_bwd_local", "tfa_bwd_alibi"], kw
    stub.calls.clear()
    ops.flash_attn_bwd(q, k, k, out, lse, out, True, softcap=50.0)
    ops.flash_attn_bwd(q, k, k, out, lse, out, True, alibi_slopes=slopes, softcap=50.0)
    assert names() == ["tfa_bwd_softcap"] * 2
    assert stub.calls[0][1][1:4] == (50.0, None, 0) and stub.calls[1][1][1:4] == (50.0, ADDR, 0)


def test_positional_slopes_still_bind_to_alibi_slopes(stub):
    import tiny_flash_attention_amd as tfa

    q = _meta(2, 256, 4, 64)                                                              # (B, N, H, D)
    slopes = _meta(4, dtype=torch.float32)
    with torch.no_grad():
        tfa.flash_attn_func(q, q, q, True, None, (-1, -1), slopes)
        tfa.flash_attn_func(q, q, q, True, None, (-1, -1), slopes, softcap=50.0)
        tfa.flash_attn_func(q, q, q, True, None, (-1, -1), softcap=50.0)
    assert [c[0] for c in stub.calls] == ["tfa_fwd_alibi", "tfa_fwd_softcap", "tfa_fwd_softcap"]
    assert stub.calls[1][1][1:3] == (50.0, ADDR) and stub.calls[2][1][1:3] == (50.0, None)
    with pytest.raises(TypeError):
        tfa.flash_attn_func(q, q, q, True, None, (-1, -1), slopes, 50.0)


def test_python_wrappers_refuse_before_any_call(stub):
    q, k = _meta(2, 4, 256, 64), _meta(2, 4, 256, 64)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="softcap"):
            ops.flash_attn_fwd(q, k, k, True, softcap=bad)
    with pytest.raises(ValueError, match="exact_max"):
        ops.flash_attn_fwd(q, k, k, True, exact_max=True, softcap=50.0)
    with pytest.raises(ValueError, match="split-KV"):
        ops.flash_attn_fwd(q, k, k, True, kv_offset=64, nk_total=512, softcap=50.0)
    with pytest.raises(ValueError, match="up to 128"):
        ops.flash_attn_fwd(_meta(1, 2, 64, 256), _meta(1, 2, 64, 256), _meta(1, 2, 64, 256), True, softcap=50.0)
    with pytest.raises(ValueError, match="float16 / bfloat16"):
        q32 = _meta(1, 2, 64, 64, dtype=torch.float32)
        ops.flash_attn_fwd(q32, q32, q32, True, softcap=50.0)
    out, lse = _meta(2, 4, 256, 64), _meta(2, 4, 256, dtype=torch.float32)
    with pytest.raises(ValueError, match="workspace"):
        ops.flash_attn_bwd(q, k, k, out, lse, out, True, workspace=True, softcap=50.0)
    assert stub.calls == []


def test_varlen_func_still_refuses_dropout():
    import tiny_flash_attention_amd as tfa

    x = torch.zeros(4, 2, 64, dtype=torch.bfloat16)
    cu = torch.tensor([0, 4], dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="dropout"):
        tfa.flash_attn_varlen_func(x, x, x, cu, cu, 4, 4, dropout_p=0.1, softcap=50.0)
    assert not math.isnan(ops._softcap(50.0, torch.bfloat16, 64))
