"""CPU tests of the packed variable-length entry points (include/tfa.h: tfa_fwd_varlen, tfa_bwd_varlen): validation codes, kernel choice and the
Python wrappers' host-side rejections.  No GPU: plans never launch, and the wrappers refuse before they touch a device."""
import ctypes as C

import pytest
import torch

from tiny_flash_attention_amd import _lib, ops
import tiny_flash_attention_amd as tfa

ADDR = 0x10000          # a 16-byte aligned stand-in for device pointers (plans never dereference them)


def fwd_params(B=4, H=8, Hk=8, D=128, max_q=1024, max_k=1024, total_q=4096, total_k=4096, causal=True, dtype=_lib.TFA_BF16, out_dtype=None):
    p = _lib.TfaVarlenFwdParams()
    p.q = p.k = p.v = p.out = p.lse = p.cu_seqlens_q = p.cu_seqlens_k = ADDR
    p.B, p.H, p.Hk, p.D = B, H, Hk, D
    p.max_seqlen_q, p.max_seqlen_k, p.total_q, p.total_k = max_q, max_k, total_q, total_k
    for name, heads in (("q_stride", H), ("k_stride", Hk), ("v_stride", Hk), ("o_stride", H)):
        arr = getattr(p, name)
        arr[0], arr[1] = D, heads * D              # (total, heads, D) contiguous: head stride D, row stride heads * D
    p.softmax_scale = 0.125
    p.is_causal = 1 if causal else 0
    p.dtype = dtype
    p.out_dtype = dtype if out_dtype is None else out_dtype
    return p


def bwd_params(B=4, H=8, Hk=8, D=128, max_q=1024, max_k=1024, total_q=4096, total_k=4096, causal=True, dtype=_lib.TFA_BF16):
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


def plan(p):
    g, b, l = C.c_int(), C.c_int(), C.c_int()
    return _lib.lib().tfa_fwd_varlen_plan(C.byref(p), C.byref(g), C.byref(b), C.byref(l)), g.value, b.value


def bwd_status(p):
    # tfa_bwd_varlen with a NULL-free but refused descriptor returns before any launch; a valid one is never passed here (it would launch)
    return _lib.lib().tfa_bwd_varlen(C.byref(p), None)


def test_symbols_exported():
    L = _lib.lib()
    for s in ("tfa_fwd_varlen", "tfa_fwd_varlen_plan", "tfa_fwd_varlen_variant", "tfa_fwd_varlen_rounding_rule", "tfa_bwd_varlen"):
        assert s in _lib.SYMBOLS
        getattr(L, s)


def test_plan_valid_and_grid():
    st, grid, block = plan(fwd_params())
    assert st == 0
    v = _lib.lib().tfa_fwd_varlen_variant(C.byref(fwd_params()))
    assert v in (30, 32)
    bm, wg = (256, 512) if v == 30 else (128, 256)
    nmb = (1024 + bm - 1) // bm
    assert block == wg and grid == 4 * 8 * ((nmb + 1) // 2)     # causal: heavy + light blocks paired per work item


@pytest.mark.parametrize("field,value,code", [
    ("D", 136, "TFA_ERR_HEAD_DIM"), ("D", 256, "TFA_ERR_HEAD_DIM"), ("D", 60, "TFA_ERR_HEAD_DIM"), ("D", 0, "TFA_ERR_HEAD_DIM"),
    ("dtype", _lib.TFA_F32, "TFA_ERR_DTYPE"), ("dtype", 7, "TFA_ERR_DTYPE"), ("out_dtype", _lib.TFA_F16, "TFA_ERR_DTYPE"),
    ("B", 0, "TFA_ERR_SHAPE"), ("H", 0, "TFA_ERR_SHAPE"), ("Hk", 0, "TFA_ERR_SHAPE"), ("Hk", 3, "TFA_ERR_SHAPE"),
    ("max_seqlen_q", 0, "TFA_ERR_SHAPE"), ("max_seqlen_k", -1, "TFA_ERR_SHAPE"), ("total_q", 0, "TFA_ERR_SHAPE"), ("total_k", 0, "TFA_ERR_SHAPE"),
    ("flags", 1, "TFA_ERR_SHAPE"), ("flags", 2, "TFA_ERR_SHAPE"), ("reserved_", 1, "TFA_ERR_SHAPE"),
    ("cu_seqlens_q", None, "TFA_ERR_NULL"), ("cu_seqlens_k", None, "TFA_ERR_NULL"), ("q", None, "TFA_ERR_NULL"),
    ("softmax_scale", 0.0, "TFA_ERR_SCALE"),
])
def test_fwd_refusals(field, value, code):
    codes = {"TFA_ERR_NULL": -1, "TFA_ERR_DTYPE": -2, "TFA_ERR_HEAD_DIM": -3, "TFA_ERR_SHAPE": -4, "TFA_ERR_STRIDE": -5, "TFA_ERR_SCALE": -8}
    p = fwd_params(dtype=_lib.TFA_BF16)
    setattr(p, field, value)
    if field == "dtype" and value == _lib.TFA_F32:
        p.out_dtype = _lib.TFA_F32
    assert plan(p)[0] == codes[code]
    assert _lib.lib().tfa_fwd_varlen_variant(C.byref(p)) == codes[code]
    assert _lib.lib().tfa_fwd_varlen_rounding_rule(C.byref(p)) == codes[code]


def test_fwd_null_params():
    assert _lib.lib().tfa_fwd_varlen_plan(None, None, None, None) == -1
    assert _lib.lib().tfa_bwd_varlen(None, None) == -1


def test_fwd_stride_refusals():
    # max_seqlen rows of one slice beyond one descriptor (2 GiB): no windowed varlen form
    p = fwd_params(H=32, Hk=32, max_q=300000, max_k=1024, total_q=300000)
    assert plan(p)[0] == -5
    p = fwd_params(H=32, Hk=32, max_q=1024, max_k=300000, total_k=300000)
    assert plan(p)[0] == -5
    p = fwd_params()
    p.q_stride[1] = 100                            # row stride below D
    assert plan(p)[0] == -5
    p = fwd_params()
    p.k_stride[0] = 4                              # head stride not 16-byte aligned
    assert plan(p)[0] == -5
    p = fwd_params()
    p.q = ADDR + 2
    assert plan(p)[0] == -6


@pytest.mark.parametrize("field,value,code", [
    ("D", 136, -3), ("dtype", _lib.TFA_F32, -2), ("grad_dtype", _lib.TFA_F16, -2), ("B", 0, -4), ("Hk", 3, -4),
    ("max_seqlen_q", 0, -4), ("total_k", 0, -4), ("flags", 1, -4), ("cu_seqlens_q", None, -1), ("cu_seqlens_k", None, -1),
    ("delta", None, -1), ("max_seqlen_k", 300000, -5),
])
def test_bwd_refusals(field, value, code):
    p = bwd_params(H=32, Hk=32)
    setattr(p, field, value)
    if field == "max_seqlen_k":
        p.total_k = value
    assert bwd_status(p) == code


@pytest.mark.parametrize("B,H,Hk,N,D", [(4, 32, 32, 4096, 128), (4, 8, 8, 1024, 64), (4, 32, 8, 4096, 128), (2, 16, 16, 2048, 128),
                                        (1, 8, 8, 4096, 128), (8, 32, 32, 512, 64), (1, 4, 4, 16384, 128), (16, 32, 32, 1024, 128)])
@pytest.mark.parametrize("causal", [False, True])
def test_variant_matches_fixed_length(B, H, Hk, N, D, causal):
    """Equal lengths: the kernel tfa_fwd picks for (B, H, Hk, N, N, D) — its key-split choices (36, 37) map to il4 (32)."""
    fixed = _lib.variant_for(B, H, Hk, N, N, D, causal)
    p = fwd_params(B=B, H=H, Hk=Hk, D=D, max_q=N, max_k=N, total_q=B * N, total_k=B * N, causal=causal)
    v = _lib.lib().tfa_fwd_varlen_variant(C.byref(p))
    assert v == (32 if fixed in (36, 37) else fixed)
    assert v in (30, 32)


@pytest.mark.parametrize("max_q,max_k", [(1, 4096), (7, 100), (100, 7), (3000, 3000), (65536, 65536)])
def test_variant_is_il8_or_il4(max_q, max_k):
    for causal in (False, True):
        p = fwd_params(B=3, H=4, Hk=2, D=64, max_q=max_q, max_k=max_k, total_q=3 * max_q, total_k=3 * max_k, causal=causal)
        assert _lib.lib().tfa_fwd_varlen_variant(C.byref(p)) in (30, 32)


def test_forced_variant():
    try:
        for v in (30, 32):
            _lib.set_variant(v)
            assert _lib.lib().tfa_fwd_varlen_variant(C.byref(fwd_params())) == v
        _lib.set_variant(17)                        # no varlen form
        assert _lib.lib().tfa_fwd_varlen_variant(C.byref(fwd_params())) == -7
    finally:
        _lib.set_variant(-1)


def test_rounding_rule():
    assert _lib.lib().tfa_fwd_varlen_rounding_rule(C.byref(fwd_params(dtype=_lib.TFA_BF16))) == _lib.RULE_FIRST_TILE
    assert _lib.lib().tfa_fwd_varlen_rounding_rule(C.byref(fwd_params(dtype=_lib.TFA_F16))) == _lib.RULE_LAZY
    assert _lib.lib().tfa_fwd_varlen_rounding_rule(C.byref(fwd_params(dtype=_lib.TFA_BF16, out_dtype=_lib.TFA_F32))) == _lib.RULE_FIRST_TILE


# ---- the Python wrappers refuse on the host, before any device work -------------------------------------------------------------

def _args(dtype=torch.bfloat16, H=4, Hk=4, D=64, total=32, B=2):
    q = torch.zeros((total, H, D), dtype=dtype)
    k = torch.zeros((total, Hk, D), dtype=dtype)
    v = torch.zeros((total, Hk, D), dtype=dtype)
    cu = torch.arange(0, total + 1, total // B, dtype=torch.int32)
    return q, k, v, cu, cu.clone()


def test_wrapper_dropout_refused():
    q, k, v, cq, ck = _args()
    with pytest.raises(NotImplementedError):
        tfa.flash_attn_varlen_func(q, k, v, cq, ck, 16, 16, 0.1)


def test_wrapper_rejections():
    q, k, v, cq, ck = _args()
    with pytest.raises(TypeError, match="float16 or bfloat16 only"):                    # fp32 inputs
        ops.flash_attn_varlen_fwd(q.float(), k.float(), v.float(), cq, ck, 16, 16)
    with pytest.raises(TypeError, match="must share dtype"):                             # mixed dtypes
        ops.flash_attn_varlen_fwd(q, k.half(), v, cq, ck, 16, 16)
    with pytest.raises(RuntimeError, match="must be a 3-D tensor"):                      # 4-D inputs
        ops.flash_attn_varlen_fwd(q[None], k[None], v[None], cq, ck, 16, 16)
    with pytest.raises(TypeError, match="cu_seqlens_q must be int32"):                  # cu_seqlens not int32
        ops.flash_attn_varlen_fwd(q, k, v, cq.long(), ck, 16, 16)
    with pytest.raises(RuntimeError, match="must both hold B \\+ 1 entries"):             # cu_seqlens of different lengths
        ops.flash_attn_varlen_fwd(q, k, v, cq, ck[:-1], 16, 16)
    with pytest.raises(RuntimeError, match="cu_seqlens_q must be a contiguous 1-D"):    # non-contiguous cu_seqlens
        ops.flash_attn_varlen_fwd(q, k, v, torch.zeros(6, dtype=torch.int32)[::2], ck, 16, 16)
    with pytest.raises(RuntimeError, match="max_seqlen_q must be a positive host integer"):   # max_seqlen: a positive host integer
        ops.flash_attn_varlen_fwd(q, k, v, cq, ck, 0, 16)
    with pytest.raises(RuntimeError, match="max_seqlen_q must be a positive host integer"):
        ops.flash_attn_varlen_fwd(q, k, v, cq, ck, torch.tensor(16), 16)
    with pytest.raises(RuntimeError, match="max_seqlen_k must be a positive host integer"):
        ops.flash_attn_varlen_fwd(q, k, v, cq, ck, 16, 2.5)
    with pytest.raises(RuntimeError, match="multiple of the K/V heads"):                 # H not a multiple of Hk
        ops.flash_attn_varlen_fwd(q, k[:, :3], v[:, :3], cq, ck, 16, 16)
    with pytest.raises(RuntimeError, match="q must have unit stride along the head dimension"):   # unit stride along D
        ops.flash_attn_varlen_fwd(q.transpose(1, 2).contiguous().transpose(1, 2), k, v, cq, ck, 16, 16)
    with pytest.raises(RuntimeError, match="q must be a CUDA tensor"):                   # host tensors: a CUDA device is required (no CPU fallback)
        ops.flash_attn_varlen_fwd(q, k, v, cq, ck, 16, 16)
    with pytest.raises(RuntimeError, match="q must be a CUDA tensor"):
        ops.flash_attn_varlen_bwd(q, k, v, q, torch.zeros(4, 32), q, cq, ck, 16, 16)


def test_package_exports():
    for n in ("flash_attn_varlen_func", "flash_attn_varlen_fwd", "flash_attn_varlen_bwd"):
        assert n in tfa.__all__ and callable(getattr(tfa, n))
