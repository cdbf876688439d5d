"""Reference-named operators over the C ABI (include/tfa.h).

Argument meaning, order, return shapes and error behaviour follow the reference's pybind
functions; the compute is the hand-written HIP kernel in csrc/.  Nothing here falls back to
PyTorch or the CPU: if the library is missing or the device is not a GPU the call raises.
"""
import ctypes as C
import functools
import math

import torch
from torch.autograd.function import once_differentiable

from . import _lib

_DT = {torch.float16: _lib.TFA_F16, torch.bfloat16: _lib.TFA_BF16}
_DT_IN = dict(_DT)
_DT_IN[torch.float32] = _lib.TFA_F32    # fp32 q,k,v: the fp32 correctness path (the reference's fp32 fixtures; tfa_fwd_f32.hip) — forward only


def _dt16(t, what):
    """dtype code of a float16 / bfloat16 tensor for the entries that have no fp32 path (backward, split-KV, raw parameter blocks)."""
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"{what}: float16 or bfloat16 only (got {t.dtype}); the fp32 path is forward-only — ops.flash_attn_fwd / tfa_fwd "
                        "with dtype = TFA_F32") from None


def _check_input(x, name):
    # CHECK_INPUT of the reference (flash_attention_cutlass/include/attention_api.cuh:12-18)
    if not x.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    if not x.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")


def _strides_bhnd(t, layout):
    """(batch, head, row) element strides of a 4-D tensor given its logical layout."""
    if layout == "bhnd":
        return t.stride(0), t.stride(1), t.stride(2)
    if layout == "bnhd":
        return t.stride(0), t.stride(2), t.stride(1)
    raise ValueError(f"unknown layout {layout!r}")


def _window(window_size, causal, nq, nk, dtype, D, extra=()):
    """FlashAttention-2's ``window_size=(left, right)`` checked and normalised as the C ABI does it (include/tfa.h, local attention): returns
    ``None`` for full / causal attention (the existing entry points run) or ``(left, right)`` for a true sliding window.  Unsupported combinations
    raise ValueError naming the limit; ``extra``: (condition, message) pairs that rule a true window out."""
    try:
        left, right = (int(w) for w in window_size)
    except (TypeError, ValueError):
        raise ValueError(f"window_size must be a pair of integers (left, right), got {window_size!r}") from None
    if left < -1 or right < -1:
        raise ValueError(f"window_size sides must be >= -1 (-1 = unbounded), got {(left, right)}")
    if causal:
        right = 0
    if left >= nk - 1:
        left = -1
    if left < 0 and right == 0:
        return None if causal else (-1, 0)
    if right >= nq - 1:
        right = -1
    if left < 0 and right < 0:
        return None
    if dtype == torch.float32:
        raise ValueError("window_size: sliding windows run on float16 / bfloat16 inputs only (no fp32 local path)")
    if D > 128:
        raise ValueError(f"window_size: sliding windows support head dims up to 128 (got {D})")
    for cond, msg in extra:
        if cond:
            raise ValueError(f"window_size: {msg}")
    return (left, right)


def _alibi(alibi_slopes, B, H, device, dtype, D, extra=()):
    """FlashAttention-2's ``alibi_slopes`` checked as the C ABI needs them (include/tfa.h, ALiBi) without touching a device: float32, shape ``(H,)`` or
    ``(B, H)`` (B: the batch, or the number of sequences of a packed call), contiguous, on ``device``.  Returns ``None`` for ``None``, else
    ``(slopes, batch_stride)`` with batch_stride 0 for ``(H,)`` and H for ``(B, H)``.  The values are never read here: the kernels load them.
    Unsupported combinations raise ValueError naming the limit; ``extra``: (condition, message) pairs that rule slopes out."""
    if alibi_slopes is None:
        return None
    if not isinstance(alibi_slopes, torch.Tensor):
        raise TypeError(f"alibi_slopes must be a float32 tensor (got {type(alibi_slopes).__name__})")
    if alibi_slopes.dtype != torch.float32:
        raise TypeError(f"alibi_slopes must be float32 (got {alibi_slopes.dtype})")
    if tuple(alibi_slopes.shape) not in ((H,), (B, H)):
        raise ValueError(f"alibi_slopes must have shape ({H},) or ({B}, {H}): one slope per query head, optionally per batch entry / sequence "
                         f"(got {tuple(alibi_slopes.shape)})")
    if not alibi_slopes.is_contiguous():
        raise ValueError("alibi_slopes must be contiguous")
    if alibi_slopes.device != device:
        raise ValueError(f"alibi_slopes must be on q's device ({device}; got {alibi_slopes.device})")
    if dtype == torch.float32:
        raise ValueError("alibi_slopes: ALiBi runs on float16 / bfloat16 inputs only (no fp32 ALiBi path)")
    if D > 128:
        raise ValueError(f"alibi_slopes: ALiBi supports head dims up to 128 (got {D})")
    for cond, msg in extra:
        if cond:
            raise ValueError(f"alibi_slopes: {msg}")
    return alibi_slopes, (H if alibi_slopes.dim() == 2 else 0)


def _softcap(softcap, dtype, D, extra=()):
    """FlashAttention-2's ``softcap`` checked as the C ABI needs it (include/tfa.h, soft-capping): a host number, 0.0 (the default) = no cap.  Returns 0.0 for
    no cap — the caller then takes the code path it took before the argument existed — else the cap as a float.  Negative, NaN and infinite values and the
    combinations the soft-capping kernels do not run raise ValueError naming the limit; ``extra``: (condition, message) pairs that rule a cap out."""
    if isinstance(softcap, torch.Tensor):
        raise TypeError("softcap must be a host number, not a tensor (nothing is read from the device)")
    cap = float(softcap)
    if cap == 0.0:
        return 0.0
    if not (cap > 0.0) or math.isinf(cap):
        raise ValueError(f"softcap must be a finite number >= 0 (0 = no cap; got {softcap})")
    if dtype == torch.float32:
        raise ValueError("softcap: soft-capping runs on float16 / bfloat16 inputs only (no fp32 soft-capping path)")
    if D > 128:
        raise ValueError(f"softcap: soft-capping supports head dims up to 128 (got {D})")
    for cond, msg in extra:
        if cond:
            raise ValueError(f"softcap: {msg}")
    return cap


def _attn_bias(attn_bias, B, H, Nq, Nk, device, dtype, D, alibi_slopes=None, softcap=0.0, extra=()):
    """``attn_bias`` checked and prepared as the C ABI needs it (include/tfa.h, dense bias) without reading its values: a 4-D tensor broadcastable to
    ``(B, H, Nq, Nk)`` — each of the first two dims 1 or full — on ``device``, of q's dtype, float32, or ``torch.bool`` under
    scaled_dot_product_attention's convention (True = attend).  Returns ``None`` for ``None``, else ``(tensor, TfaAttnBias)``: the tensor the kernels read
    (kept alive by the caller) and its struct, broadcast dims as stride 0.  A bool mask becomes 0 / -inf in q's dtype (one elementwise op); a tensor whose
    base or strides miss the kernels' alignment (16-byte base, unit stride along keys, other strides multiples of 8 elements) is copied once into a buffer
    whose row stride is Nk rounded up to 8 — a prepared tensor passes through unchanged.  Everything else raises by name before any launch."""
    if attn_bias is None:
        return None
    if not isinstance(attn_bias, torch.Tensor):
        raise TypeError(f"attn_bias must be a tensor (got {type(attn_bias).__name__})")
    if attn_bias.dtype not in (torch.bool, torch.float32, dtype):
        raise TypeError(f"attn_bias must be torch.bool, float32 or q's dtype {dtype} (got {attn_bias.dtype})")
    if attn_bias.dim() != 4 or attn_bias.shape[0] not in (1, B) or attn_bias.shape[1] not in (1, H) or tuple(attn_bias.shape[2:]) != (Nq, Nk):
        raise ValueError(f"attn_bias must have shape ({B} or 1, {H} or 1, {Nq}, {Nk}): 4-D, broadcastable over batch and query heads "
                         f"(got {tuple(attn_bias.shape)})")
    if attn_bias.device != device:
        raise ValueError(f"attn_bias must be on q's device ({device}; got {attn_bias.device})")
    if attn_bias.requires_grad:
        raise RuntimeError("attn_bias requires grad, but the bias gets no gradient (a learned bias would silently stop training): detach it")
    if alibi_slopes is not None:
        raise ValueError("attn_bias: not together with alibi_slopes (add the ALiBi term to the bias instead)")
    if isinstance(softcap, torch.Tensor) or float(softcap) != 0.0:
        raise ValueError("attn_bias: not together with softcap")
    if dtype == torch.float32:
        raise ValueError("attn_bias: the bias runs on float16 / bfloat16 inputs only (no fp32 bias path)")
    if D > 128:
        raise ValueError(f"attn_bias: the bias supports head dims up to 128 (got {D})")
    for cond, msg in extra:
        if cond:
            raise ValueError(f"attn_bias: {msg}")
    t = attn_bias
    if t.dtype == torch.bool:
        t = torch.where(t, torch.zeros((), dtype=dtype, device=device), torch.full((), float("-inf"), dtype=dtype, device=device))
    for d in (0, 1):                                     # (an expanded dim is a broadcast one)
        if t.shape[d] > 1 and t.stride(d) == 0:
            t = t.narrow(d, 0, 1)
    sizes, st = t.shape, t.stride()
    aligned = (t.data_ptr() % 16 == 0 and (Nk == 1 or st[3] == 1) and (Nq == 1 or (st[2] % 8 == 0 and st[2] >= Nk)) and
               all(sizes[d] == 1 or (st[d] >= 0 and st[d] % 8 == 0) for d in (0, 1)))
    if not aligned:
        rs = (Nk + 7) // 8 * 8
        buf = torch.zeros((sizes[0], sizes[1], Nq, rs), dtype=t.dtype, device=device)
        buf[..., :Nk].copy_(t)
        t = buf[..., :Nk]
        st = t.stride()
    bi = _lib.TfaAttnBias()
    bi.bias = t.data_ptr()
    bi.dtype = _lib.TFA_F32 if t.dtype == torch.float32 else _DT[t.dtype]
    bi.reserved_ = 0
    bi.stride[0] = 0 if sizes[0] == 1 else st[0]
    bi.stride[1] = 0 if sizes[1] == 1 else st[1]
    bi.stride[2] = 0 if Nq == 1 else st[2]
    return t, bi


def _slopes_arg(alibi):
    """(pointer or None, batch stride) of checked slopes for a _softcap entry point, which takes NULL as "no bias"."""
    return (None, 0) if alibi is None else (alibi[0].data_ptr(), alibi[1])


def _alibi_window(win, is_causal):
    """The window an ALiBi entry point is given: a true window as it is, else (-1, -1) / (-1, 0) — the ALiBi kernels run every mask."""
    return win if win is not None else ((-1, 0) if is_causal else (-1, -1))


def _call_form(base, p, stream, win, alibi, cap, is_causal, bias=None):
    """Calls the entry point of one attention form on the parameter block p: ``base`` (tfa_fwd, tfa_fwd_varlen, tfa_bwd, tfa_bwd_varlen) with the suffix and the
    extra arguments of the checked bias / softcap / slopes / window — _bias (never with a cap or slopes), _softcap before _alibi before _local, else ``base`` itself."""
    if bias is not None:
        suffix, extra = "_bias", (C.byref(bias[1]), *_alibi_window(win, is_causal))
    elif cap:
        suffix, extra = "_softcap", (cap, *_slopes_arg(alibi), *_alibi_window(win, is_causal))
    elif alibi is not None:
        suffix, extra = "_alibi", (alibi[0].data_ptr(), alibi[1], *_alibi_window(win, is_causal))
    elif win is not None:
        suffix, extra = "_local", (win[0], win[1])
    else:
        suffix, extra = "", ()
    _lib.check(getattr(_lib.lib(), base + suffix)(C.byref(p), *extra, C.c_void_p(stream)))


def flash_attn_fwd(q, k, v, is_causal=False, softmax_scale=None, *, layout="bhnd", out_f32=False,
                   return_lse=True, out=None, kv_offset=0, nk_total=None, auto_split=False, exact_max=False, window_size=(-1, -1), attn_bias=None,
                   softcap=0.0, alibi_slopes=None):
    """General forward: q (B,H,Nq,D) / k,v (B,Hk,Nk,D) for ``layout='bhnd'`` or
    (B,N,H,D) for ``layout='bnhd'``; any batch/head/row strides, unit stride along D.
    Returns ``(out, lse)``; ``out`` has q's shape (fp32 when ``out_f32``), ``lse`` is (B,H,Nq) fp32.
    Maps onto tfa_fwd (include/tfa.h); semantics per flash_attention_c/csrc/attn.cpp:101-169 and
    flash_attention_cutlass/csrc/flash_attention.cu:536-630.  ``auto_split``: decode-like shapes (few query rows, long K/V)
    go through tfa_fwd_splitkv with the chunk count tfa_fwd_suggest_splits names (what the reference-named entry points do).
    ``exact_max``: TFA_FWD_EXACT_MAX — P is rounded to 16 bits at the reference's own points (exact running row maximum per
    KV tile, main_torch_only.py:240-260); head dims up to 128.
    ``window_size=(left, right)``: FlashAttention-2's local (sliding-window) attention — key j is visible to row i iff
    i + (Nk - Nq) - left <= j <= i + (Nk - Nq) + right, -1 = unbounded, ``is_causal`` forces right = 0 (tfa_fwd_local).
    ``alibi_slopes``: FlashAttention-2's ALiBi — float32 (H,) or (B, H) on q's device; ``-slope[b, h] * |i + (Nk - Nq) - j|`` is added to the scaled
    scores before the mask and the softmax, and the returned LSE includes it (tfa_fwd_alibi; the slopes are read by the kernels only; with any mask
    or window; not with ``exact_max`` or split-KV arguments, ``auto_split`` is ignored).
    ``softcap``: FlashAttention-2's tanh logit capping, a host float, 0.0 = none: the scaled scores x become ``softcap * tanh(x / softcap)`` FIRST, then the
    ALiBi bias is added, then the mask applies; the LSE is that of the capped scores (tfa_fwd_softcap; tanh within 2^-20; float16 / bfloat16, head dims up to
    128, any mask or window, with or without slopes; not with ``exact_max`` or split-KV arguments, ``auto_split`` is ignored; negative / NaN / inf: ValueError).
    ``attn_bias``: a dense additive bias / mask, scaled_dot_product_attention's ``attn_mask`` — a 4-D tensor broadcastable to (B, H, Nq, Nk) (each of the first
    two dims 1 or full; indexed by the QUERY head under GQA) of q's dtype or float32, added to the scaled scores before the mask and the softmax; the LSE
    includes it; ``-inf`` entries mask, a row without a finite score gives out = 0 and lse = +inf; ``+inf`` and NaN are undefined.  A ``torch.bool`` tensor
    is a mask (True = attend) and is converted to 0 / -inf in q's dtype with one elementwise op; a tensor whose base or strides miss the kernels' alignment
    (16-byte base, unit stride along keys, other strides multiples of 8 elements) is copied once into a padded buffer.  The values are read by the kernels
    only (tfa_fwd_bias): no host copy, no synchronisation.  float16 / bfloat16, head dims up to 128, any mask or window; not with ``alibi_slopes``,
    ``softcap``, ``exact_max`` or split-KV arguments (ValueError), ``auto_split`` is ignored; a bias that requires grad is refused (RuntimeError): it gets
    no gradient."""
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        if not t.is_cuda:
            raise RuntimeError(f"{n} must be a CUDA tensor")
        if t.dim() != 4:
            raise RuntimeError(f"{n} must be 4-D")
        if t.stride(3) != 1:
            raise RuntimeError(f"{n} must have unit stride along the head dimension")
    if q.dtype not in _DT_IN or k.dtype != q.dtype or v.dtype != q.dtype:
        raise TypeError(f"q,k,v must share dtype float16, bfloat16 or float32 (got {q.dtype}, {k.dtype}, {v.dtype})")
    if q.dtype == torch.float32 and (exact_max or (out is not None and out.dtype != torch.float32)):
        raise TypeError("float32 q,k,v: the fp32 correctness path returns float32 and has no 16-bit rounding points (exact_max does not apply)")
    if k.device != q.device or v.device != q.device:
        raise RuntimeError("q,k,v must be on the same device")
    if layout == "bhnd":
        B, H, Nq, D = q.shape
        Bk, Hk, Nk, Dk = k.shape
    else:
        B, Nq, H, D = q.shape
        Bk, Nk, Hk, Dk = k.shape
    if k.shape != v.shape or Bk != B or Dk != D:
        raise RuntimeError(f"shape mismatch: q {tuple(q.shape)} k {tuple(k.shape)} v {tuple(v.shape)}")
    if softmax_scale is None:
        softmax_scale = 1.0 / math.sqrt(D)
    win = _window(window_size, is_causal, Nq, Nk, q.dtype, D,
                  extra=((exact_max, "no exact_max form of the local kernels"), (kv_offset != 0 or nk_total is not None, "no split-KV / partial passes")))
    if win == (-1, 0):                               # (the causal mask itself: tfa_fwd with is_causal)
        win, is_causal = None, True
    bias = _attn_bias(attn_bias, B, H, Nq, Nk, q.device, q.dtype, D, alibi_slopes, softcap,
                      extra=((exact_max, "no exact_max form of the bias kernels"), (kv_offset != 0 or nk_total is not None, "no split-KV / partial passes")))
    alibi = _alibi(alibi_slopes, B, H, q.device, q.dtype, D,
                   extra=((exact_max, "no exact_max form of the ALiBi kernels"), (kv_offset != 0 or nk_total is not None, "no split-KV / partial passes")))
    cap = _softcap(softcap, q.dtype, D,
                   extra=((exact_max, "no exact_max form of the soft-capping kernels"), (kv_offset != 0 or nk_total is not None, "no split-KV / partial passes")))

    if out is None:
        out = torch.empty(q.shape, dtype=torch.float32 if out_f32 else q.dtype, device=q.device)
    else:   # a caller-owned result buffer: the kernel writes q.shape elements at out's strides — check before launching
        if not isinstance(out, torch.Tensor) or out.shape != q.shape:
            raise RuntimeError(f"out must be a tensor shaped like q {tuple(q.shape)}")
        if out.device != q.device:
            raise RuntimeError("out must be on q's device")
        if out.dtype not in (q.dtype, torch.float32):
            raise RuntimeError(f"out must be {q.dtype} or float32 (got {out.dtype})")
        if out.stride(3) != 1:
            raise RuntimeError("out must have unit stride along the head dimension")
    lse = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device) if return_lse else None

    p = _lib.TfaFwdParams()
    p.q, p.k, p.v, p.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    p.lse = lse.data_ptr() if lse is not None else None
    p.B, p.H, p.Hk, p.Nq, p.Nk, p.D = B, H, Hk, Nq, Nk, D
    for name, t in (("q_stride", q), ("k_stride", k), ("v_stride", v), ("o_stride", out)):
        s = _strides_bhnd(t, layout)
        arr = getattr(p, name)
        arr[0], arr[1], arr[2] = s
    p.softmax_scale = float(softmax_scale)
    p.is_causal = 1 if is_causal else 0
    p.dtype = _DT_IN[q.dtype]
    p.out_dtype = _lib.TFA_F32 if out.dtype == torch.float32 else _DT[out.dtype]
    p.kv_offset = int(kv_offset)                     # split-KV: k, v are keys [kv_offset, kv_offset+Nk) of nk_total
    p.nk_total = 0 if nk_total is None else int(nk_total)
    p.flags = _lib.TFA_FWD_EXACT_MAX if exact_max else 0
    L = _lib.lib()
    # tfa_fwd_splitkv's merge writes a dense (B,H,Nq,D) result: gate on the exact strides it checks (is_contiguous() ignores the
    # strides of size-1 dims, and Nq == 1 is the very shape auto-split targets)
    dense_out = (out.stride(3) == 1 and out.stride(2) == D and out.stride(1) == Nq * D and out.stride(0) == H * Nq * D)
    splits = L.tfa_fwd_suggest_splits(C.byref(p)) if (auto_split and layout == "bhnd" and dense_out and win is None and alibi is None and not cap and
                                                       bias is None) else 1
    with torch.cuda.device(q.device):
        stream = torch.cuda.current_stream().cuda_stream
        if splits > 1:
            need = L.tfa_fwd_splitkv_workspace(C.byref(p), int(splits))
            if need < 0:
                _lib.check(int(need))
            ws = torch.empty((int(need),), dtype=torch.float32, device=q.device)
            _lib.check(L.tfa_fwd_splitkv(C.byref(p), int(splits), ws.data_ptr(), C.c_void_p(stream)))
        else:
            _call_form("tfa_fwd", p, stream, win, alibi, cap, is_causal, bias)
    return out, lse


def merge_partials(o_parts, lse_parts, out_dtype=torch.bfloat16):
    """Split-KV merge (tfa_merge): ``o_parts`` (P,B,H,Nq,D) fp32 and ``lse_parts`` (P,B,H,Nq) fp32 are partial
    attention results of the same queries over disjoint key chunks (``flash_attn_fwd(..., out_f32=True,
    kv_offset=..., nk_total=...)``); returns ``(out, lse)`` of the whole key sequence.  The rule is the reference's
    v1 merge (flash_attention_py/tiny_flash_attn.py:63-68) in LSE form."""
    if not o_parts.is_cuda or o_parts.dtype != torch.float32 or lse_parts.dtype != torch.float32:
        raise RuntimeError("o_parts / lse_parts must be fp32 CUDA tensors")
    o_parts, lse_parts = o_parts.contiguous(), lse_parts.contiguous()
    P, D = o_parts.shape[0], o_parts.shape[-1]
    rows = lse_parts[0].numel()
    if o_parts[0].numel() != rows * D or lse_parts.shape[0] != P:
        raise RuntimeError("shape mismatch between o_parts and lse_parts")
    out = torch.empty(o_parts.shape[1:], dtype=out_dtype, device=o_parts.device)
    lse = torch.empty(lse_parts.shape[1:], dtype=torch.float32, device=o_parts.device)
    code = _lib.TFA_F32 if out_dtype == torch.float32 else _DT[out_dtype]
    with torch.cuda.device(o_parts.device):
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.lib().tfa_merge(o_parts.data_ptr(), lse_parts.data_ptr(), P, rows, D, rows * D, rows,
                                        out.data_ptr(), code, lse.data_ptr(), C.c_void_p(stream)))
    return out, lse


def flash_attn_fwd_splitkv(q, k, v, is_causal=False, softmax_scale=None, *, splits=2, return_lse=True, native=True):
    """The forward as `splits` partial passes over contiguous key chunks (multiples of 64 keys) + tfa_merge;
    (B,H,N,D) layout, out contiguous.  ``native=True``: tfa_fwd_splitkv — ONE launch whose grid carries a copy of the
    work per chunk (what decode-like shapes need to fill the chip), partials in a scratch tensor.
    ``native=False``: one tfa_fwd call per chunk driven from Python (what dist.kv_sharded_forward does per rank)."""
    Nk = k.shape[2]
    if native:
        B, H, Nq, D = q.shape
        if softmax_scale is None:
            softmax_scale = 1.0 / math.sqrt(D)
        out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        lse = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
        p = make_params(q, k, v, out, lse, is_causal, softmax_scale)
        L = _lib.lib()
        need = L.tfa_fwd_splitkv_workspace(C.byref(p), int(splits))
        if need < 0:
            _lib.check(int(need))
        ws = torch.empty((int(need),), dtype=torch.float32, device=q.device)
        with torch.cuda.device(q.device):
            stream = torch.cuda.current_stream().cuda_stream
            _lib.check(L.tfa_fwd_splitkv(C.byref(p), int(splits), ws.data_ptr(), C.c_void_p(stream)))
        return (out, lse) if return_lse else out
    step = ((Nk + splits - 1) // splits + 63) // 64 * 64
    o_parts, l_parts = [], []
    for lo in range(0, Nk, step):
        hi = min(Nk, lo + step)
        o, l = flash_attn_fwd(q, k[:, :, lo:hi], v[:, :, lo:hi], is_causal, softmax_scale, out_f32=True, kv_offset=lo, nk_total=Nk)
        o_parts.append(o)
        l_parts.append(l)
    out, lse = merge_partials(torch.stack(o_parts), torch.stack(l_parts), q.dtype)
    return (out, lse) if return_lse else out


def make_params(q, k, v, out, lse, is_causal, softmax_scale, layout="bhnd"):
    """Build a TfaFwdParams for existing buffers (used by bench.py / tfa_fwd_time)."""
    p = _lib.TfaFwdParams()
    p.q, p.k, p.v, p.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    p.lse = lse.data_ptr() if lse is not None else None
    if layout == "bhnd":
        B, H, Nq, D = q.shape
        _, Hk, Nk, _ = k.shape
    else:
        B, Nq, H, D = q.shape
        _, Nk, Hk, _ = k.shape
    p.B, p.H, p.Hk, p.Nq, p.Nk, p.D = B, H, Hk, Nq, Nk, D
    for name, t in (("q_stride", q), ("k_stride", k), ("v_stride", v), ("o_stride", out)):
        s = _strides_bhnd(t, layout)
        arr = getattr(p, name)
        arr[0], arr[1], arr[2] = s
    p.softmax_scale = float(softmax_scale)
    p.is_causal = 1 if is_causal else 0
    p.dtype = _dt16(q, "make_params (q, k, v)")
    p.out_dtype = _lib.TFA_F32 if out.dtype == torch.float32 else _dt16(out, "make_params (out)")
    return p


def make_bwd_params(q, k, v, out, lse, dout, dq, dk, dv, delta, is_causal, softmax_scale, layout="bhnd"):
    """Build a TfaBwdParams for existing buffers."""
    p = _lib.TfaBwdParams()
    p.q, p.k, p.v, p.out, p.dout = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), dout.data_ptr()
    p.lse, p.delta = lse.data_ptr(), delta.data_ptr()
    p.dq, p.dk, p.dv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    if layout == "bhnd":
        B, H, Nq, D = q.shape
        _, Hk, Nk, _ = k.shape
    else:
        B, Nq, H, D = q.shape
        _, Nk, Hk, _ = k.shape
    p.B, p.H, p.Hk, p.Nq, p.Nk, p.D = B, H, Hk, Nq, Nk, D
    for name, t in (("q_stride", q), ("k_stride", k), ("v_stride", v), ("o_stride", out), ("do_stride", dout),
                    ("dq_stride", dq), ("dk_stride", dk), ("dv_stride", dv)):
        s = _strides_bhnd(t, layout)
        arr = getattr(p, name)
        arr[0], arr[1], arr[2] = s
    p.softmax_scale = float(softmax_scale)
    p.is_causal = 1 if is_causal else 0
    p.dtype = _dt16(q, "backward (q, k, v)")
    p.grad_dtype = _lib.TFA_F32 if dq.dtype == torch.float32 else _dt16(dq, "backward (gradients)")
    return p


def flash_attn_bwd(q, k, v, out, lse, dout, is_causal=False, softmax_scale=None, *, layout="bhnd", grad_f32=False, workspace=None, window_size=(-1, -1),
                   attn_bias=None, softcap=0.0, alibi_slopes=None):
    """Backward of ``flash_attn_fwd``: returns ``(dq, dk, dv)`` shaped like q, k, v (fp32 when ``grad_f32``).
    ``out`` and ``lse`` are the forward's results for the same q, k, v; ``dout`` is the upstream gradient
    (shape/dtype of ``out``).  The reference has no backward — it only saves the LSE for one
    (flash_attention_cutlass/csrc/flash_attention.cu:353-354,614-623); maps onto tfa_bwd (include/tfa.h).
    ``workspace``: None (default: the O(N)-memory 7-GEMM form), True (allocate tfa_bwd_workspace_bytes of scratch for this call)
    or a caller-owned uint8 / any-dtype CUDA tensor of at least that many bytes: tfa_bwd then keeps dS and executes 5 GEMMs.
    ``window_size``: the forward's sliding window (tfa_bwd_local; no workspace form).
    ``alibi_slopes``: the forward's ALiBi slopes (tfa_bwd_alibi; no workspace form); they receive no gradient.
    ``softcap``: the forward's soft cap (tfa_bwd_softcap; no workspace form): dS is multiplied by 1 - tanh^2 on its way to dq and dk; no gradient for it.
    ``attn_bias``: the forward's dense bias / mask (tfa_bwd_bias; no workspace form; checked and prepared as in ``flash_attn_fwd``); it receives no gradient."""
    for t, n in ((q, "q"), (k, "k"), (v, "v"), (out, "out"), (dout, "dout")):
        if not t.is_cuda:
            raise RuntimeError(f"{n} must be a CUDA tensor")
        if t.dim() != 4 or t.stride(3) != 1:
            raise RuntimeError(f"{n} must be 4-D with unit stride along the head dimension")
    if q.dtype not in _DT or any(t.dtype != q.dtype for t in (k, v, out, dout)):
        raise TypeError("q,k,v,out,dout must share dtype float16 or bfloat16")
    if out.shape != q.shape or dout.shape != q.shape or k.shape != v.shape:
        raise RuntimeError("shape mismatch")
    D = q.shape[-1]
    if softmax_scale is None:
        softmax_scale = 1.0 / math.sqrt(D)
    lse_shape = (q.shape[0], q.shape[1], q.shape[2]) if layout == "bhnd" else (q.shape[0], q.shape[2], q.shape[1])   # (B,H,Nq)
    if not lse.is_cuda or lse.device != q.device or lse.dtype != torch.float32 or tuple(lse.shape) != lse_shape:
        raise RuntimeError(f"lse must be the forward's float32 {lse_shape} tensor on q's device "
                           f"(got {lse.dtype} {tuple(lse.shape)} on {lse.device})")
    if any(t.device != q.device for t in (k, v, out, dout)):
        raise RuntimeError("q,k,v,out,dout must be on the same device")
    nq, nk = (q.shape[2], k.shape[2]) if layout == "bhnd" else (q.shape[1], k.shape[1])
    win = _window(window_size, is_causal, nq, nk, q.dtype, D, extra=((workspace is not None and workspace is not False, "no dS-workspace form"),))
    if win == (-1, 0):
        win, is_causal = None, True
    bias = _attn_bias(attn_bias, q.shape[0], lse_shape[1], nq, nk, q.device, q.dtype, D, alibi_slopes, softcap,
                      extra=((workspace is not None and workspace is not False, "no dS-workspace form"),))
    alibi = _alibi(alibi_slopes, q.shape[0], lse_shape[1], q.device, q.dtype, D,
                   extra=((workspace is not None and workspace is not False, "no dS-workspace form"),))
    cap = _softcap(softcap, q.dtype, D, extra=((workspace is not None and workspace is not False, "no dS-workspace form"),))
    lse = lse.contiguous()
    gdt = torch.float32 if grad_f32 else q.dtype
    dq = torch.empty(q.shape, dtype=gdt, device=q.device)
    dk = torch.empty(k.shape, dtype=gdt, device=q.device)
    dv = torch.empty(v.shape, dtype=gdt, device=q.device)
    delta = torch.empty(lse.shape, dtype=torch.float32, device=q.device)
    p = make_bwd_params(q, k, v, out, lse, dout, dq, dk, dv, delta, is_causal, softmax_scale, layout)
    if workspace is not None and workspace is not False:
        need = bwd_workspace_bytes(p)
        if workspace is True:
            workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=q.device)
        if not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or workspace.device != q.device or not workspace.is_contiguous():
            raise RuntimeError("workspace must be True or a contiguous CUDA tensor on q's device")
        p.workspace = workspace.data_ptr()
        p.workspace_bytes = workspace.numel() * workspace.element_size()
    with torch.cuda.device(q.device):
        stream = torch.cuda.current_stream().cuda_stream
        _call_form("tfa_bwd", p, stream, win, alibi, cap, is_causal, bias)
    return dq, dk, dv


def bwd_workspace_bytes(p):
    """tfa_bwd_workspace_bytes for a TfaBwdParams (0: the 5-GEMM form does not apply to this problem)."""
    L = _lib.lib()
    L.tfa_bwd_workspace_bytes.restype = C.c_longlong
    n = L.tfa_bwd_workspace_bytes(C.byref(p))
    if n < 0:
        _lib.check(int(n))
    return int(n)


# ---------------------------------------------------------------------------------------------
# the reference's three operator entry points
# ---------------------------------------------------------------------------------------------
def flash_attention_v2_cutlass(q, k, v, is_causal, softmax_scale):
    """``attention_cutlass.flash_attention_v2_cutlass(q, k, v, is_causal, softmax_scale) -> [out, lse]``
    (flash_attention_cutlass/csrc/flash_attention.cu:741-772).  q,k,v: contiguous CUDA
    (B,H,N,D) fp16/bf16; out like q; lse (B,H,N) fp32.  All five arguments are positional, as
    in the reference binding (no py::arg, attention_api.cpp:6-10).  Launches on the current
    stream and does not synchronise (the reference blocks; its callers synchronise anyway)."""
    _check_input(q, "q")
    _check_input(k, "k")
    _check_input(v, "v")
    out, lse = flash_attn_fwd(q, k, v, bool(is_causal), float(softmax_scale), auto_split=True)
    return [out, lse]


def flash_attention_v2_cuda(q, k, v):
    """``attention_cuda.flash_attention_v2_cuda(q, k, v) -> out``: non-causal, scale fixed to
    1/sqrt(D) inside (flash_attention_cuda/csrc/flash_attention.cu:375-424, :389)."""
    _check_input(q, "q")
    _check_input(k, "k")
    _check_input(v, "v")
    out, _ = flash_attn_fwd(q, k, v, False, 1.0 / math.sqrt(q.shape[-1]), return_lse=False, auto_split=True)
    return out


# the reference exports three names from attention_cuda; all compute the same function
# (flash_attention_cuda/csrc/attention_api.cpp:6-14) — here they share the one kernel.
flash_attention_v1_cuda = flash_attention_v2_cuda
self_attention_cuda = flash_attention_v2_cuda


def flash_attn(q, k, v, is_causal, softmax_scale):
    """``_kernels.flash_attn(q, k, v, is_causal, softmax_scale) -> out``
    (flash_attention_c/csrc/attn.cpp:237-262).  Same math as the CPU sibling, including its
    bottom-right-aligned causal mask for Nq != Nk (attn.cpp:121-124) and strided inputs
    (attn.cpp:171-203); tensors live on the GPU: fp16 / bf16 (the MFMA kernels) or fp32 (the reference's own fixture dtype: the fp32
    correctness path, fp32 arithmetic end to end)."""
    out, _ = flash_attn_fwd(q, k, v, bool(is_causal), float(softmax_scale), return_lse=False, auto_split=True)
    return out


# naive_attn computes the same function by a different route in the reference
# (attn.cpp:35-98); the GPU path has one kernel.
naive_attn = flash_attn


def _once_differentiable(backward):
    """``torch.autograd.function.once_differentiable`` for a backward whose result also depends on tensors the forward SAVED: the gradients come out of ctypes
    launches, with no graph behind them, so under ``create_graph=True`` a second derivative would silently be that of a constant.  torch's decorator attaches
    its error node only when an incoming gradient requires grad; the gradient of a linear loss does not, yet dq, dk, dv still depend on q, k, v — so under
    ``create_graph=True`` (the only time a backward runs with grad mode on) the incoming gradients are handed on as views that require grad, and
    differentiating anything that depends on the results raises RuntimeError."""
    once = once_differentiable(backward)

    @functools.wraps(backward)
    def wrapper(ctx, *grads):
        if torch.is_grad_enabled():
            grads = tuple(g.detach().requires_grad_() if isinstance(g, torch.Tensor) and not g.requires_grad else g for g in grads)
        return once(ctx, *grads)

    return wrapper


def _kernel_dout(dout, row_dim):
    """The upstream gradient autograd hands over, as tfa_bwd / tfa_bwd_varlen read it.  The C ABI's own rule (csrc/tfa_bwd_api.hip: check_strides, check_bwd):
    unit stride along D, every other stride >= 0 and a multiple of 8 elements, the row stride (dim ``row_dim``) >= D, a 16-byte base.  A gradient that meets
    it is passed on AS IT IS — ``out.transpose(1, 2)``'s, or the zero batch / head stride of ``out.sum(0)`` / ``out.sum(2)``: the kernels form every address
    from base + b * stride_b + h * stride_h + row * stride_n and read such a gradient to the bits of its dense copy.  One that misses it — the zero row stride
    of ``out.sum(1)``, the odd strides and offset base behind a ``torch.cat`` — is copied once.  The handed tensor may be shared with other consumers of the
    graph: it is read, never written (the copy is this call's own)."""
    D = dout.shape[-1]
    st = dout.stride()
    if st[-1] == 1 and all(s >= 0 and s % 8 == 0 for s in st[:-1]) and st[row_dim] >= D and dout.data_ptr() % 16 == 0:
        return dout
    return dout.clone(memory_format=torch.contiguous_format)


class _FlashAttnBNHD(torch.autograd.Function):
    """autograd glue for ``flash_attn_func``: forward = tfa_fwd, backward = tfa_bwd, both on (B,N,H,D) views."""

    @staticmethod
    def forward(ctx, q, k, v, causal, softmax_scale, window_size=(-1, -1), attn_bias=None, softcap=0.0, alibi_slopes=None):
        if attn_bias is not None:                        # (checked and prepared once: the backward reads the tensor the forward read)
            attn_bias = _attn_bias(attn_bias, q.shape[0], q.shape[2], q.shape[1], k.shape[1], q.device, q.dtype, q.shape[3], alibi_slopes, softcap)[0]
        out, lse = flash_attn_fwd(q, k, v, causal, softmax_scale, layout="bnhd", window_size=window_size, attn_bias=attn_bias, alibi_slopes=alibi_slopes,
                                  softcap=softcap)
        ctx.save_for_backward(q, k, v, out, lse, alibi_slopes, attn_bias)   # (the slopes and the bias, or None: they get no gradient)
        ctx.causal, ctx.scale, ctx.window, ctx.softcap = causal, softmax_scale, window_size, softcap
        return out

    @staticmethod
    @_once_differentiable
    def backward(ctx, dout):
        q, k, v, out, lse, slopes, bias = ctx.saved_tensors
        dout = _kernel_dout(dout, 1)
        dq, dk, dv = flash_attn_bwd(q, k, v, out, lse, dout, ctx.causal, ctx.scale, layout="bnhd", window_size=ctx.window, attn_bias=bias,
                                    alibi_slopes=slopes, softcap=ctx.softcap)
        return dq, dk, dv, None, None, None, None, None, None   # (causal, scale, window, bias, softcap, slopes: no gradient)


def _positional_slopes(extra, alibi_slopes, name):
    """``alibi_slopes`` given as the one positional argument behind ``window_size`` (where it stood before ``softcap`` existed) or as a keyword."""
    if len(extra) > 1 or (extra and alibi_slopes is not None):
        raise TypeError(f"{name}: at most one positional argument behind window_size (alibi_slopes), and not together with the keyword")
    return extra[0] if extra else alibi_slopes


def flash_attn_func(q, k, v, causal=False, softmax_scale=None, window_size=(-1, -1), *extra, attn_bias=None, softcap=0.0, alibi_slopes=None):
    """(B,N,H,D)-layout entry with the signature the reference's scripts use for comparison
    (flash_attention_cutlass/test.py:71-76, flash_attention_py/main_torch_only.py:304);
    supports GQA/MQA (fewer K/V heads).  Differentiable (like the official function the reference
    compares against): when an input requires grad the backward runs tfa_bwd.  ``window_size=(left, right)``: FlashAttention-2's local
    (sliding-window) attention, -1 = unbounded, ``causal`` forces right = 0 (tfa_fwd_local / tfa_bwd_local).  ``alibi_slopes``: FlashAttention-2's
    ALiBi, float32 (H,) or (B, H): ``-slope * |i + (Nk - Nq) - j|`` added to the scaled scores (tfa_fwd_alibi / tfa_bwd_alibi); no gradient for them.
    ``softcap``: FlashAttention-2's tanh logit capping (Gemma-2 style), a host float, 0.0 = none: scaled scores x become ``softcap * tanh(x / softcap)`` before
    the ALiBi bias and the mask (cap, then bias, then mask); differentiable through the cap (tfa_fwd_softcap / tfa_bwd_softcap), no gradient for the value itself.
    ``softcap`` is keyword-only; ``alibi_slopes`` stays the last parameter and may still be passed as the positional argument behind ``window_size``.
    ``attn_bias`` (keyword-only): a dense additive bias / mask as scaled_dot_product_attention's ``attn_mask`` — 4-D, broadcastable to (B, H, Nq, Nk) with each
    of the first two dims 1 or full (the QUERY head under GQA), of q's dtype or float32, added to the scaled scores before ``causal`` / ``window_size``;
    ``-inf`` masks, a fully masked row gives 0; ``+inf`` / NaN are undefined.  A ``torch.bool`` tensor (True = attend) is converted to 0 / -inf in q's dtype
    with one elementwise op, and a tensor that misses the kernels' alignment (16-byte base, strides multiples of 8 elements, unit stride along keys) is
    copied once into a padded buffer.  Differentiable in q, k, v (tfa_fwd_bias / tfa_bwd_bias); the bias itself gets no gradient and one that requires
    grad is refused (RuntimeError).  Not with ``alibi_slopes`` or ``softcap`` (ValueError).  ``None``: the call above, unchanged."""
    alibi_slopes = _positional_slopes(extra, alibi_slopes, "flash_attn_func")
    window_size = tuple(window_size)
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        return _FlashAttnBNHD.apply(q, k, v, bool(causal), softmax_scale, window_size, attn_bias, softcap, alibi_slopes)
    out, _ = flash_attn_fwd(q, k, v, causal, softmax_scale, layout="bnhd", return_lse=False, window_size=window_size, attn_bias=attn_bias,
                            alibi_slopes=alibi_slopes, softcap=softcap)
    return out


# ---------------------------------------------------------------------------------------------
# packed variable-length batches: the cu_seqlens form of FlashAttention-2's flash_attn_varlen_func (tfa_fwd_varlen / tfa_bwd_varlen)
# ---------------------------------------------------------------------------------------------

def _check_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, extra=()):
    """Host-side checks of a packed call — everything that needs no device read (cu_seqlens itself is only read by the kernels).
    Returns B (the sequence count)."""
    for t, n in ((q, "q"), (k, "k"), (v, "v")) + tuple(extra):
        if not isinstance(t, torch.Tensor) or t.dim() != 3:
            raise RuntimeError(f"{n} must be a 3-D tensor (total rows, heads, head dim)")
        if t.stride(2) != 1:
            raise RuntimeError(f"{n} must have unit stride along the head dimension")
    if q.dtype == torch.float32:
        raise TypeError("packed variable-length attention: float16 or bfloat16 only (no fp32 varlen path)")
    if q.dtype not in _DT or k.dtype != q.dtype or v.dtype != q.dtype:
        raise TypeError(f"q,k,v must share dtype float16 or bfloat16 (got {q.dtype}, {k.dtype}, {v.dtype})")
    if k.shape != v.shape or k.shape[2] != q.shape[2]:
        raise RuntimeError(f"shape mismatch: q {tuple(q.shape)} k {tuple(k.shape)} v {tuple(v.shape)}")
    if q.shape[1] % k.shape[1] != 0:
        raise RuntimeError(f"the query heads ({q.shape[1]}) must be a multiple of the K/V heads ({k.shape[1]})")
    for t, n in ((cu_seqlens_q, "cu_seqlens_q"), (cu_seqlens_k, "cu_seqlens_k")):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{n} must be a tensor")
        if t.dtype != torch.int32:
            raise TypeError(f"{n} must be int32 (got {t.dtype})")
        if t.dim() != 1 or not t.is_contiguous() or t.numel() < 2:
            raise RuntimeError(f"{n} must be a contiguous 1-D tensor of B + 1 >= 2 entries")
    if cu_seqlens_q.numel() != cu_seqlens_k.numel():
        raise RuntimeError(f"cu_seqlens_q and cu_seqlens_k must both hold B + 1 entries ({cu_seqlens_q.numel()} vs {cu_seqlens_k.numel()})")
    for m, n in ((max_seqlen_q, "max_seqlen_q"), (max_seqlen_k, "max_seqlen_k")):
        if isinstance(m, torch.Tensor) or isinstance(m, bool) or int(m) != m or int(m) <= 0:
            raise RuntimeError(f"{n} must be a positive host integer (got {m!r})")
    for t, n in ((q, "q"), (k, "k"), (v, "v")) + tuple(extra) + ((cu_seqlens_q, "cu_seqlens_q"), (cu_seqlens_k, "cu_seqlens_k")):
        if not t.is_cuda:
            raise RuntimeError(f"{n} must be a CUDA tensor")
        if t.device != q.device:
            raise RuntimeError(f"{n} must be on q's device")
    return cu_seqlens_q.numel() - 1


def _check_varlen_paged(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, block_table, window_size, is_causal, softcap, alibi_slopes):
    """Host-side checks of a packed call over a page pool (``block_table`` given): everything that needs no device read, refused by name before any library call."""
    name = "flash_attn_varlen_func(block_table=...)"
    if not isinstance(q, torch.Tensor) or q.dim() != 3:
        raise RuntimeError("q must be a 3-D tensor (total rows, heads, head dim)")
    for t, n in ((k, "k"), (v, "v")):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError(f"{name}: {n} must be the 4-D page pool (num_pages, page_size, Hk, D)")
    if q.dtype == torch.float32:
        raise TypeError("packed variable-length attention: float16 or bfloat16 only (no fp32 varlen path)")
    if q.dtype not in _DT:
        raise TypeError(f"{name}: float16 or bfloat16 only (got {q.dtype})")
    fp8s = tuple(getattr(torch, n) for n in ("float8_e4m3fn", "float8_e5m2", "float8_e4m3fnuz", "float8_e5m2fnuz") if hasattr(torch, n))
    if k.dtype in fp8s or v.dtype in fp8s:
        raise TypeError(f"{name}: fp8 page pools are not supported (got {k.dtype}, {v.dtype}); flash_attn_with_kvcache reads an fp8 cache")
    if k.dtype != q.dtype or v.dtype != q.dtype:
        raise TypeError(f"{name}: k and v must have q's dtype {q.dtype} (got {k.dtype}, {v.dtype})")
    total_q, H, D = q.shape
    if D > 128:
        raise ValueError(f"{name}: head dims up to 128 (got {D})")
    if D % 8 != 0 or D < 8:
        raise ValueError(f"{name}: the head dim must be a multiple of 8 (got {D})")
    if k.shape != v.shape or k.shape[3] != D:
        raise ValueError(f"{name}: k and v must have one shape (num_pages, page_size, Hk, {D}) (got {tuple(k.shape)}, {tuple(v.shape)})")
    num_pages, page_size, Hk, _ = k.shape
    if num_pages <= 0 or page_size <= 0 or page_size % 64 != 0:
        raise ValueError(f"{name}: the page size must be a positive multiple of 64 and the pool hold a page (got {page_size}, {num_pages} pages)")
    if Hk <= 0 or H % Hk != 0:
        raise ValueError(f"{name}: the K/V heads ({Hk}) must divide the query heads ({H})")
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        if t.stride(-1) != 1:
            raise ValueError(f"{name}: {n} must have unit stride along the head dim")
    for t, n in ((cu_seqlens_q, "cu_seqlens_q"), (cu_seqlens_k, "cu_seqlens_k")):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{n} must be a tensor")
        if t.dtype != torch.int32:
            raise TypeError(f"{n} must be int32 (got {t.dtype})")
        if t.dim() != 1 or not t.is_contiguous() or t.numel() < 2:
            raise RuntimeError(f"{n} must be a contiguous 1-D tensor of B + 1 >= 2 entries")
    if cu_seqlens_q.numel() != cu_seqlens_k.numel():
        raise RuntimeError(f"cu_seqlens_q and cu_seqlens_k must both hold B + 1 entries ({cu_seqlens_q.numel()} vs {cu_seqlens_k.numel()})")
    B = cu_seqlens_q.numel() - 1
    for m, n in ((max_seqlen_q, "max_seqlen_q"), (max_seqlen_k, "max_seqlen_k")):
        if isinstance(m, torch.Tensor) or isinstance(m, bool) or int(m) != m or int(m) <= 0:
            raise RuntimeError(f"{n} must be a positive host integer (got {m!r})")
    if not isinstance(block_table, torch.Tensor) or block_table.dtype != torch.int32 or block_table.dim() != 2 or block_table.shape[0] != B or block_table.shape[1] < 1:
        raise ValueError(f"{name}: block_table must be an int32 tensor of shape ({B}, max_blocks)")
    if block_table.device != q.device or block_table.stride(1) != 1:
        raise ValueError(f"{name}: block_table must be on q's device with unit stride along max_blocks")
    for t, n in ((q, "q"), (k, "k"), (v, "v"), (cu_seqlens_q, "cu_seqlens_q"), (cu_seqlens_k, "cu_seqlens_k")):
        if not t.is_cuda:
            raise RuntimeError(f"{n} must be a CUDA tensor")
        if t.device != q.device:
            raise RuntimeError(f"{n} must be on q's device")
    # the combinations that are a follow-up: a true window, a cap, slopes ((-1, -1) and (-1, 0) windows are full / causal attention as everywhere)
    win = _window(window_size, is_causal, int(max_seqlen_q), int(max_seqlen_k), q.dtype, D,
                  extra=((True, "sliding windows are not implemented over a page pool (block_table)"),))
    if isinstance(softcap, torch.Tensor) or float(softcap) != 0.0:
        raise ValueError(f"{name}: softcap is not implemented over a page pool (block_table)")
    if alibi_slopes is not None:
        raise ValueError(f"{name}: alibi_slopes is not implemented over a page pool (block_table)")
    return B, (True if win == (-1, 0) else bool(is_causal))


def flash_attn_varlen_fwd(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, is_causal=False, softmax_scale=None, *,
                          out_f32=False, return_lse=True, out=None, window_size=(-1, -1), block_table=None, softcap=0.0, alibi_slopes=None):
    """Packed variable-length forward (tfa_fwd_varlen, include/tfa.h): q (total_q, H, D), k / v (total_k, Hk, D), sequence b is rows
    [cu_seqlens_q[b], cu_seqlens_q[b+1]) of q and [cu_seqlens_k[b], cu_seqlens_k[b+1]) of k, v (device int32, B + 1 entries, never read on the host).
    Causal masking per sequence, bottom-right aligned.  Returns ``(out, lse)``: ``out`` shaped like q (fp32 when ``out_f32``), ``lse`` fp32 (H, total_q).
    Rows outside every sequence are not written (a caller-provided ``out`` keeps them).  ``window_size``: FlashAttention-2's sliding window per
    sequence (tfa_fwd_varlen_local).  ``alibi_slopes``: ALiBi, float32 (H,) or (B, H) with B the number of sequences; the distance is taken per sequence
    (tfa_fwd_varlen_alibi).  ``softcap``: tanh logit capping of the scaled scores before the bias and the mask, 0.0 = none (tfa_fwd_varlen_softcap).
    ``block_table`` (keyword-only; tfa_fwd_varlen_paged): paged K/V — k / v are the page pool (num_pages, page_size, Hk, D), any page / row / head strides, page_size a
    multiple of 64; ``block_table`` int32 (B, max_blocks) on the device; sequence b has cu_seqlens_k[b+1] - cu_seqlens_k[b] keys (only the difference is used), key j in
    row j % page_size of page block_table[b, j // page_size].  Not with a true window, softcap or alibi_slopes (ValueError).  ``None``: the call above, unchanged."""
    if block_table is not None:
        B, is_causal = _check_varlen_paged(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, block_table, window_size, is_causal, softcap,
                                           alibi_slopes)
        total_q, H, D = q.shape
        total_k, Hk = 0, k.shape[2]
        win, alibi, cap = None, None, 0.0
    else:
        _check_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k)
        B = cu_seqlens_q.numel() - 1
        total_q, H, D = q.shape
        total_k, Hk, _ = k.shape
    if softmax_scale is None:
        softmax_scale = 1.0 / math.sqrt(D)
    if block_table is None:
        win = _window(window_size, is_causal, int(max_seqlen_q), int(max_seqlen_k), q.dtype, D)
        if win == (-1, 0):
            win, is_causal = None, True
        alibi = _alibi(alibi_slopes, B, H, q.device, q.dtype, D)
        cap = _softcap(softcap, q.dtype, D)
    if out is None:
        out = torch.empty(q.shape, dtype=torch.float32 if out_f32 else q.dtype, device=q.device)
    else:
        if not isinstance(out, torch.Tensor) or out.shape != q.shape or out.device != q.device:
            raise RuntimeError(f"out must be a tensor shaped like q {tuple(q.shape)} on q's device")
        if out.dtype not in (q.dtype, torch.float32):
            raise RuntimeError(f"out must be {q.dtype} or float32 (got {out.dtype})")
        if out.stride(2) != 1:
            raise RuntimeError("out must have unit stride along the head dimension")
    lse = torch.empty((H, total_q), dtype=torch.float32, device=q.device) if return_lse else None
    p = _lib.TfaVarlenFwdParams()
    p.q, p.k, p.v, p.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    p.lse = lse.data_ptr() if lse is not None else None
    p.cu_seqlens_q, p.cu_seqlens_k = cu_seqlens_q.data_ptr(), cu_seqlens_k.data_ptr()
    p.B, p.H, p.Hk, p.D = B, H, Hk, D
    p.max_seqlen_q, p.max_seqlen_k, p.total_q, p.total_k = int(max_seqlen_q), int(max_seqlen_k), total_q, total_k
    for name, t in (("q_stride", q), ("o_stride", out)) + ((("k_stride", k), ("v_stride", v)) if block_table is None else ()):
        arr = getattr(p, name)
        arr[0], arr[1] = t.stride(1), t.stride(0)
    p.softmax_scale = float(softmax_scale)
    p.is_causal = 1 if is_causal else 0
    p.dtype = _DT[q.dtype]
    p.out_dtype = _lib.TFA_F32 if out.dtype == torch.float32 else _DT[out.dtype]
    if block_table is not None:
        for name, t in (("k_stride", k), ("v_stride", v)):          # the pool (num_pages, page_size, Hk, D): head, row — the page strides go into pg
            arr = getattr(p, name)
            arr[0], arr[1] = t.stride(2), t.stride(1)
        pg = _lib.TfaPagedKv()
        pg.block_table, pg.table_stride, pg.max_blocks = block_table.data_ptr(), block_table.stride(0), block_table.shape[1]
        pg.page_size, pg.num_pages = k.shape[1], k.shape[0]
        pg.k_page_stride, pg.v_page_stride = k.stride(0), v.stride(0)
        with torch.cuda.device(q.device):
            stream = torch.cuda.current_stream().cuda_stream
            _lib.check(_lib.lib().tfa_fwd_varlen_paged(C.byref(p), C.byref(pg), C.c_void_p(stream)))
        return out, lse
    with torch.cuda.device(q.device):
        stream = torch.cuda.current_stream().cuda_stream
        _call_form("tfa_fwd_varlen", p, stream, win, alibi, cap, is_causal)
    return out, lse


def flash_attn_varlen_bwd(q, k, v, out, lse, dout, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, is_causal=False, softmax_scale=None, *,
                          grad_f32=False, window_size=(-1, -1), softcap=0.0, alibi_slopes=None):
    """Backward of ``flash_attn_varlen_fwd`` (tfa_bwd_varlen): returns ``(dq, dk, dv)`` shaped like q, k, v (fp32 when ``grad_f32``); for GQA dk / dv
    are summed over the query heads of each K/V head within each sequence.  Rows outside every sequence get zero gradients: the kernels never write
    them, so the three results are allocated zeroed (one memset of dq, dk and dv per call).  ``window_size``, ``alibi_slopes``, ``softcap``: the forward's."""
    _check_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, extra=((out, "out"), (dout, "dout")))
    if out.shape != q.shape or dout.shape != q.shape or out.dtype != q.dtype or dout.dtype != q.dtype:
        raise RuntimeError("out and dout must be shaped like q, in q's dtype")
    B = cu_seqlens_q.numel() - 1
    total_q, H, D = q.shape
    total_k, Hk, _ = k.shape
    if softmax_scale is None:
        softmax_scale = 1.0 / math.sqrt(D)
    if not isinstance(lse, torch.Tensor) or not lse.is_cuda or lse.device != q.device or lse.dtype != torch.float32 or tuple(lse.shape) != (H, total_q):
        raise RuntimeError(f"lse must be the forward's float32 {(H, total_q)} tensor on q's device")
    win = _window(window_size, is_causal, int(max_seqlen_q), int(max_seqlen_k), q.dtype, D)
    if win == (-1, 0):
        win, is_causal = None, True
    alibi = _alibi(alibi_slopes, B, H, q.device, q.dtype, D)
    cap = _softcap(softcap, q.dtype, D)
    lse = lse.contiguous()
    gdt = torch.float32 if grad_f32 else q.dtype
    dq = torch.zeros(q.shape, dtype=gdt, device=q.device)
    dk = torch.zeros(k.shape, dtype=gdt, device=q.device)
    dv = torch.zeros(v.shape, dtype=gdt, device=q.device)
    delta = torch.empty((H, total_q), dtype=torch.float32, device=q.device)
    p = _lib.TfaVarlenBwdParams()
    p.q, p.k, p.v, p.out, p.dout = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), dout.data_ptr()
    p.lse, p.delta = lse.data_ptr(), delta.data_ptr()
    p.dq, p.dk, p.dv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    p.cu_seqlens_q, p.cu_seqlens_k = cu_seqlens_q.data_ptr(), cu_seqlens_k.data_ptr()
    p.B, p.H, p.Hk, p.D = B, H, Hk, D
    p.max_seqlen_q, p.max_seqlen_k, p.total_q, p.total_k = int(max_seqlen_q), int(max_seqlen_k), total_q, total_k
    for name, t in (("q_stride", q), ("k_stride", k), ("v_stride", v), ("o_stride", out), ("do_stride", dout),
                    ("dq_stride", dq), ("dk_stride", dk), ("dv_stride", dv)):
        arr = getattr(p, name)
        arr[0], arr[1] = t.stride(1), t.stride(0)
    p.softmax_scale = float(softmax_scale)
    p.is_causal = 1 if is_causal else 0
    p.dtype = _DT[q.dtype]
    p.grad_dtype = _lib.TFA_F32 if grad_f32 else _DT[q.dtype]
    with torch.cuda.device(q.device):
        stream = torch.cuda.current_stream().cuda_stream
        _call_form("tfa_bwd_varlen", p, stream, win, alibi, cap, is_causal)
    return dq, dk, dv


class _FlashAttnVarlen(torch.autograd.Function):
    """autograd glue for ``flash_attn_varlen_func``: forward = tfa_fwd_varlen, backward = tfa_bwd_varlen."""

    @staticmethod
    def forward(ctx, q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal, softmax_scale, window_size=(-1, -1), softcap=0.0,
                alibi_slopes=None):
        out, lse = flash_attn_varlen_fwd(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal, softmax_scale, window_size=window_size,
                                         alibi_slopes=alibi_slopes, softcap=softcap)
        ctx.save_for_backward(q, k, v, out, lse, cu_seqlens_q, cu_seqlens_k, alibi_slopes)   # (the slopes, or None: they get no gradient)
        ctx.args = (max_seqlen_q, max_seqlen_k, causal, softmax_scale, window_size, softcap)
        return out

    @staticmethod
    @_once_differentiable
    def backward(ctx, dout):
        q, k, v, out, lse, cu_q, cu_k, slopes = ctx.saved_tensors
        max_q, max_k, causal, scale, window, softcap = ctx.args
        dout = _kernel_dout(dout, 0)
        dq, dk, dv = flash_attn_varlen_bwd(q, k, v, out, lse, dout, cu_q, cu_k, max_q, max_k, causal, scale, window_size=window, alibi_slopes=slopes,
                                           softcap=softcap)
        return dq, dk, dv, None, None, None, None, None, None, None, None, None


def flash_attn_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, dropout_p=0.0, softmax_scale=None, causal=False,
                           window_size=(-1, -1), *extra, block_table=None, softcap=0.0, alibi_slopes=None):
    """Packed variable-length attention with FlashAttention-2's positional signature (flash_attn_varlen_func): q (total_q, H, D), k / v
    (total_k, Hk, D), cu_seqlens_q / _k device int32 (B + 1), max_seqlen_q / _k host integers.  Differentiable: when an input requires grad the
    backward runs tfa_bwd_varlen.  Dropout is not supported (``dropout_p`` must be 0).  ``window_size=(left, right)``: FlashAttention-2's sliding
    window per sequence, -1 = unbounded, ``causal`` forces right = 0.  ``alibi_slopes``: ALiBi, float32 (H,) or (B, H), B = the number of sequences.
    ``softcap``: tanh logit capping, a host float, 0.0 = none: cap on the scaled scores, then the bias, then the mask (tfa_fwd_varlen_softcap / tfa_bwd_varlen_softcap).
    ``softcap`` is keyword-only; ``alibi_slopes`` may still be passed as the positional argument behind ``window_size``.
    ``block_table`` (keyword-only): paged K/V, FlashAttention-2's chunked prefill over a page pool — k / v are (num_pages, page_size, Hk, D) with page_size a
    multiple of 64 (a (num_pages, Hk, page_size, D) pool works as a permuted view), ``block_table`` int32 (B, max_blocks) on the device; sequence b attends its
    cu_seqlens_k[b+1] - cu_seqlens_k[b] keys (only the difference is used; clamped on the device to max_seqlen_k and to max_blocks * page_size), key j being row
    j % page_size of page block_table[b, j // page_size] (entries clamped into the pool).  Neither the lengths nor the table are read on the host: no
    synchronisation, capturable in a graph.  ``causal`` is bottom-right aligned per sequence — new tokens see the whole prefix and each other causally.  Whatever
    the pool holds behind a sequence's length (page tails, unreferenced pages, NaN) never reaches a result.  Forward only: an input that requires grad raises
    RuntimeError.  Not with a true ``window_size``, ``softcap`` or ``alibi_slopes`` (ValueError), nor fp8 pools (TypeError).  The path works on 128- / 256-row
    query blocks: built for prefill; for decode-shaped batches (one new row per sequence) it is correct but ``flash_attn_with_kvcache`` is the call to use."""
    alibi_slopes = _positional_slopes(extra, alibi_slopes, "flash_attn_varlen_func")
    if dropout_p != 0.0:
        raise NotImplementedError("flash_attn_varlen_func: dropout is not supported (dropout_p must be 0)")
    window_size = tuple(window_size)
    if block_table is not None:
        if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (q, k, v)):
            raise RuntimeError("flash_attn_varlen_func(block_table=...) is not differentiable: an input requires grad (run it under torch.no_grad() or detach "
                               "the inputs)")
        out, _ = flash_attn_varlen_fwd(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal, softmax_scale, return_lse=False,
                                       window_size=window_size, alibi_slopes=alibi_slopes, softcap=softcap, block_table=block_table)
        return out
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        return _FlashAttnVarlen.apply(q, k, v, cu_seqlens_q, cu_seqlens_k, int(max_seqlen_q), int(max_seqlen_k), bool(causal), softmax_scale, window_size,
                                      softcap, alibi_slopes)
    out, _ = flash_attn_varlen_fwd(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal, softmax_scale, return_lse=False,
                                   window_size=window_size, alibi_slopes=alibi_slopes, softcap=softcap)
    return out


def _kvcache_params(q, k_cache, v_cache, out, lse, cache_seqlens, block_table, k_new, v_new, softmax_scale, causal):
    """A TfaKvcacheParams for FlashAttention-2's layouts: q / out (B, Nq, H, D) (out: any 4-D strides given as (B, H, Nq, D)), the caches
    (B, Nk_max, Hk, D) or paged (num_pages, page_size, Hk, D), k_new / v_new (B, n_new, Hk, D)."""
    p = _lib.TfaKvcacheParams()
    B, Nq, H, D = q.shape
    Hk = k_cache.shape[2]
    p.q, p.out = q.data_ptr(), out.data_ptr()
    p.lse = lse.data_ptr() if lse is not None else None
    p.k_cache, p.v_cache = k_cache.data_ptr(), v_cache.data_ptr()
    p.cache_seqlens = cache_seqlens.data_ptr()
    p.B, p.H, p.Hk, p.Nq, p.D = B, H, Hk, Nq, D
    if block_table is not None:
        p.block_table = block_table.data_ptr()
        p.block_table_stride = block_table.stride(0)
        p.page_size, p.num_pages = k_cache.shape[1], k_cache.shape[0]
        p.capacity = block_table.shape[1] * k_cache.shape[1]
    else:
        p.block_table = None
        p.capacity = k_cache.shape[1]
    for name, t in (("q_stride", q), ("k_stride", k_cache), ("v_stride", v_cache)):
        arr = getattr(p, name)
        arr[0], arr[1], arr[2] = t.stride(0), t.stride(2), t.stride(1)          # (B, N, H, D) tensors: batch / page, head, row
    p.o_stride[0], p.o_stride[1], p.o_stride[2] = out.stride(0), out.stride(1), out.stride(2)   # out is handed over as (B, H, Nq, D)
    if k_new is not None:
        p.k_new, p.v_new, p.n_new = k_new.data_ptr(), v_new.data_ptr(), k_new.shape[1]
        for name, t in (("knew_stride", k_new), ("vnew_stride", v_new)):
            arr = getattr(p, name)
            arr[0], arr[1], arr[2] = t.stride(0), t.stride(2), t.stride(1)
    p.softmax_scale = float(softmax_scale)
    p.is_causal = 1 if causal else 0
    p.dtype = _DT[q.dtype]
    return p


def _kvcache_checks(name, q, k_cache, v_cache, k, v, cache_seqlens, block_table, num_splits, pack_gqa, k_descale, v_descale, B, H, D, packed_q):
    """The checks the 4-D form of flash_attn_with_kvcache and its packed form (``packed_q``: q (total_q, H, D), B = cu_seqlens_q.numel() - 1) share — dtype, head
    dim, fp8 pairing, descales, block_table, capacity, k / v, grad, cache_seqlens, num_splits, pack_gqa — in the order their refusals come; where a form has a check
    or a wording of its own between two shared ones, it stands here under ``packed_q``.  Returns (fp8, Hk, capacity, cache_seqlens as a device tensor, num_splits)."""
    is_b = " — B = cu_seqlens_q.numel() - 1" if packed_q else ""    # behind a shape that names B
    is_b_ = is_b + " —" if packed_q else ""                         # ... in the middle of a sentence
    if q.dtype == torch.float32:
        raise ValueError(f"{name}: float16 / bfloat16 inputs only (no fp32 K/V-cache path)")
    if q.dtype not in _DT:
        raise TypeError(f"{name}: float16 or bfloat16 only (got {q.dtype})")
    if packed_q and q.shape[0] <= 0:
        raise ValueError(f"{name}: q holds no row")
    if D > 128:
        raise ValueError(f"{name}: head dims up to 128 (got {D})")
    if D % 8 != 0 or D < 8:
        raise ValueError(f"{name}: the head dim must be a multiple of 8 (got {D})")
    fp8 = k_cache.dtype == torch.float8_e4m3fn and v_cache.dtype == torch.float8_e4m3fn
    if not fp8 and (k_cache.dtype != q.dtype or v_cache.dtype != q.dtype):
        raise TypeError(f"{name}: q, k_cache and v_cache must share one dtype, or both caches be torch.float8_e4m3fn (got {q.dtype}, {k_cache.dtype}, "
                        f"{v_cache.dtype}; float8_e5m2 and float8_e4m3fnuz caches are not supported)")
    if fp8 and D % 16 != 0:
        raise ValueError(f"{name}: with an fp8 cache the head dim must be a multiple of 16 (got {D})")
    if not fp8 and (k_descale is not None or v_descale is not None):
        raise ValueError(f"{name}: k_descale / v_descale belong to a torch.float8_e4m3fn cache (got a {k_cache.dtype} cache)")
    if k_cache.shape != v_cache.shape or k_cache.shape[3] != D:
        raise ValueError(f"{name}: k_cache and v_cache must have one shape (..., Hk, {D}) (got {tuple(k_cache.shape)}, {tuple(v_cache.shape)})")
    Hk = k_cache.shape[2]
    if Hk <= 0 or H % Hk != 0:
        raise ValueError(f"{name}: the K/V heads ({Hk}) must divide the query heads ({H})")
    for n, t in (("k_descale", k_descale), ("v_descale", v_descale)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError(f"{name}: {n} must be a float32 tensor")
        if tuple(t.shape) != (B, Hk) or t.device != q.device:
            raise ValueError(f"{name}: {n} must have shape ({B}, {Hk}){is_b_} on q's device (got {tuple(t.shape)} on {t.device})")
    if packed_q:
        if q.stride(2) != 1 or k_cache.stride(3) != 1 or v_cache.stride(3) != 1:
            raise ValueError(f"{name}: q, k_cache and v_cache must have unit stride along the head dim")
        if (q.stride(0) * 2) % 16 != 0 or (q.stride(1) * 2) % 16 != 0:
            raise ValueError(f"{name}: the rows of q must be 16-byte aligned (strides {q.stride(0)}, {q.stride(1)} elements)")
    else:
        for n, t in (("q", q), ("k_cache", k_cache), ("v_cache", v_cache)):
            if t.stride(3) != 1:
                raise ValueError(f"{name}: {n} must have unit stride along the head dim")
    if block_table is not None:
        if not isinstance(block_table, torch.Tensor) or block_table.dtype != torch.int32 or block_table.dim() != 2 or block_table.shape[0] != B:
            raise ValueError(f"{name}: block_table must be an int32 tensor of shape ({B}, max_blocks){is_b}")
        if block_table.device != q.device or block_table.stride(1) != 1:
            raise ValueError(f"{name}: block_table must be on q's device with unit stride along max_blocks")
        if k_cache.shape[1] % 64 != 0 or k_cache.shape[1] <= 0:
            raise ValueError(f"{name}: the page size must be a positive multiple of 64 (got {k_cache.shape[1]})")
        capacity = block_table.shape[1] * k_cache.shape[1]
    else:
        if k_cache.shape[0] != B:
            batch = f"the batch size cu_seqlens_q.numel() - 1 = {B}" if packed_q else f"q's batch size {B}"
            raise ValueError(f"{name}: a contiguous cache must have {batch} (got {k_cache.shape[0]}); cache_batch_idx is not implemented")
        capacity = k_cache.shape[1]
    if capacity <= 0:
        raise ValueError(f"{name}: the cache holds no key")
    if (k is None) != (v is None):                        # (the packed form has refused k / v by now: kvcache_append_varlen is its append)
        raise ValueError(f"{name}: k and v must be given together")
    if k is not None:
        if cache_seqlens is None:
            raise ValueError(f"{name}: k / v are appended at cache_seqlens, which must then be given")
        for n, t in (("k", k), ("v", v)):
            if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[0] != B or t.shape[2] != Hk or t.shape[3] != D or t.shape[1] < 1:
                raise ValueError(f"{name}: {n} must have shape ({B}, n_new, {Hk}, {D})")
            if t.dtype != q.dtype or t.stride(3) != 1 or t.device != q.device:
                raise ValueError(f"{name}: {n} must have q's dtype and device and unit stride along the head dim")
        if k.shape != v.shape:
            raise ValueError(f"{name}: k and v must have one shape")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (q, k_cache, v_cache, k, v)):
        raise RuntimeError(f"{name} is not differentiable: an input requires grad (run it under torch.no_grad() or detach the inputs)")
    if cache_seqlens is None:
        cache_seqlens = torch.full((B,), capacity, dtype=torch.int32, device=q.device)
    elif isinstance(cache_seqlens, int):
        cache_seqlens = torch.full((B,), int(cache_seqlens), dtype=torch.int32, device=q.device)
    elif (not isinstance(cache_seqlens, torch.Tensor) or cache_seqlens.dtype != torch.int32 or tuple(cache_seqlens.shape) != (B,)
          or not cache_seqlens.is_contiguous() or cache_seqlens.device != q.device):
        raise ValueError(f"{name}: cache_seqlens must be a contiguous int32 tensor of shape ({B},){is_b_} on q's device, a host int, or None")
    num_splits = int(num_splits)
    if num_splits < 0:
        raise ValueError(f"{name}: num_splits must be >= 0 (0 = automatic; got {num_splits})")
    if pack_gqa is not None and pack_gqa is not True and pack_gqa is not False:
        raise TypeError(f"{name}: pack_gqa must be None, True or False (got {pack_gqa!r})")
    return fp8, Hk, capacity, cache_seqlens, num_splits


def _kvcache_fp8_arg(fp8, k_descale, v_descale):
    """The ``const tfa_kvcache_fp8*`` of a call: the TfaKvcacheFp8 of an e4m3 cache by reference (a None descale = 1.0), or None — NULL — for a 16-bit cache."""
    if not fp8:
        return None
    p8 = _lib.TfaKvcacheFp8()
    p8.format = _lib.TFA_KV_E4M3
    for ptr, strides, t in (("k_descale", p8.k_descale_stride, k_descale), ("v_descale", p8.v_descale_stride, v_descale)):
        if t is not None:
            setattr(p8, ptr, t.data_ptr())
            strides[0], strides[1] = t.stride(0), t.stride(1)
    return C.byref(p8)


def _kvcache_launch(suggest, workspace, launch, num_splits, device):
    """The tail of every K/V-cache call, over its entry-point family: ``suggest()`` answers ``num_splits=0``, ``workspace(splits)`` sizes the fp32 workspace (a
    negative answer is the call's refusal), ``launch(splits, workspace pointer or None, stream)`` runs on the current stream of ``device``."""
    if num_splits == 0:
        num_splits = max(1, int(suggest()))
    need = workspace(num_splits)
    if need < 0:
        _lib.check(int(need))
    ws = torch.empty((int(need),), dtype=torch.float32, device=device) if need > 0 else None
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(launch(num_splits, ws.data_ptr() if ws is not None else None, C.c_void_p(stream)))


def flash_attn_with_kvcache(q, k_cache, v_cache, k=None, v=None, cache_seqlens=None, block_table=None, softmax_scale=None, causal=False,
                            num_splits=0, return_softmax_lse=False, *, rotary_cos=None, rotary_sin=None, cache_batch_idx=None, cache_leftpad=None,
                            window_size=(-1, -1), softcap=0.0, alibi_slopes=None, pack_gqa=None, cu_seqlens_q=None, max_seqlen_q=None, tree_mask=None,
                            scheduler_metadata=None, sliding_window=None, k_descale=None, v_descale=None):
    """FlashAttention-2's ``flash_attn_with_kvcache`` (tfa_fwd_kvcache): one inference step over a K/V cache whose lengths live on the device.

    ``q`` (B, Nq, H, D); ``k_cache`` / ``v_cache`` (B, Nk_max, Hk, D) with any strides and unit stride along D, or paged (num_blocks, page_size, Hk, D)
    with ``block_table`` (B, max_blocks) int32 on the device (page_size a multiple of 64); ``cache_seqlens`` (B,) int32 on the device — never read on the
    host, so the call does not synchronise and can be captured in a graph —, a host int (broadcast) or None (the full capacity).  ``k`` / ``v``
    (B, n_new, Hk, D): appended IN PLACE at positions cache_seqlens[b] + t first (rows beyond the capacity are dropped), then attended;
    ``cache_seqlens`` itself is not advanced.  ``causal``: bottom-right aligned per sequence.  ``num_splits``: key chunks per sequence (0 = the library's
    suggestion from host-known sizes); the chunks are cut from each sequence's own length on the device.  GQA / MQA decode (Nq == 1) streams K / V once
    per K/V head; Nq > 1 runs unpacked (K / V once per query head) unless ``pack_gqa=True``.
    ``pack_gqa`` (keyword-only, FlashAttention-3's): a scheduling choice that never changes the definition of the result.  None (the default): the rule above, through
    the entry points the call always used.  True (tfa_fwd_kvcache_pack, TFA_PACK_GQA_ON): with Hk < H and H / Hk <= 128 the Nq * H / Hk rows (position t, head g) of a
    K/V head run as position-major rows of one problem — K / V stream once per K/V head while Nq * H / Hk <= 128, causal visibility stays per position — at any
    Nq; otherwise the unpacked call.  False (TFA_PACK_GQA_OFF): unpacked, also at Nq == 1.  With True / False ``num_splits=0`` asks the library for the split count
    of that geometry.  Anything else raises TypeError.  Measured (H32 Hk8 D128 bf16, 16384 keys, Nq 1..8,
    contiguous / paged, 16-bit / fp8: profiles/kvcache_packgqa_bench.txt): True is 1.5-1.6x (B = 1), 2.8-3.7x (B = 8) and 3.4-3.6x (B = 64) faster than False and slower at no shape of
    that table; other shapes were not measured.
    Returns ``out`` (B, Nq, H, D) — with more than one chunk a transposed view of the dense (B, H, Nq, D) result the merge writes — and with
    ``return_softmax_lse`` also ``lse`` (B, H, Nq) fp32.  Not differentiable: an input that requires grad raises.
    An fp8 cache (tfa_fwd_kvcache_fp8): ``k_cache`` and ``v_cache`` of dtype ``torch.float8_e4m3fn`` with ``k_descale`` / ``v_descale``, float32 device
    tensors of shape (B, Hk) with any strides (an ``expand``ed per-tensor scale works), None = 1.0; with a paged cache they are still indexed by the sequence.
    ``q``, ``k`` / ``v`` and ``out`` keep q's 16-bit dtype.  The result is attention over the exactly decoded cache: scores scaled by ``k_descale[b, hk]``, the
    output by ``v_descale[b, hk]`` in fp32; Q and P are not quantised.  ``k`` / ``v`` are quantised on the device as they are appended —
    ``rne_e4m3fn(clamp(x / descale, -448, 448))`` — and attended as quantised.  The descales are read by the kernels only (no synchronisation; a captured step sees
    values overwritten in place) and must be finite and > 0.  The head dim must be a multiple of 16.
    ``cu_seqlens_q`` / ``max_seqlen_q`` (keyword-only, FlashAttention-3's; tfa_fwd_kvcache_varlen): packed ragged query rows — the call for a unified batch of
    decode rows and chunked-prefill rows.  ``q`` is then (total_q, H, D) with any row and head strides, unit stride along D and 16-byte aligned rows;
    ``cu_seqlens_q`` a contiguous int32 device tensor of B + 1 entries, never read on the host; ``max_seqlen_q`` a positive host int (required: it sizes the
    grid).  B = cu_seqlens_q.numel() - 1 must be the batch of a contiguous cache, the rows of ``block_table``, of ``cache_seqlens`` and of the descales.  Sequence
    b owns the rows [q0_b, q0_b + nq_b), q0_b = clamp(cu_seqlens_q[b], 0, total_q), nq_b = clamp(cu_seqlens_q[b+1] - cu_seqlens_q[b], 0, min(max_seqlen_q,
    total_q - q0_b)), and attends keys [0, len_b), len_b = clamp(cache_seqlens[b], 0, capacity): ``cache_seqlens`` INCLUDES the rows appended for this step (pass
    ``cache_seqlens_before + (cu_seqlens_q[1:] - cu_seqlens_q[:-1])``, a device op).  ``causal``: key j is visible to row t of sequence b iff
    j <= t + (len_b - nq_b).  A row that sees no key gives out = 0, lse = +inf; nq_b = 0 is legal; rows of out / lse that belong to no sequence are unspecified.
    ``k`` / ``v`` must be None (ValueError: ``kvcache_append_varlen`` is the append for packed rows).  ``pack_gqa``: None and True pack whenever Hk < H and
    H / Hk <= 128, False runs unpacked (as do H == Hk and H / Hk > 128).  ``num_splits=0`` asks tfa_fwd_kvcache_varlen_suggest_splits.  Returns ``out``
    (total_q, H, D), a transposed view of the dense (H, total_q, D) buffer the kernel or the merge writes, and ``lse`` (H, total_q) fp32.  Paged and contiguous
    caches, fp8 caches with descales, zero fill behind the lengths, no host synchronisation, graph capture and "not differentiable": as above.  The grid is sized
    by ``max_seqlen_q``: one long prefill chunk in a batch of decode rows makes most work items empty (each costs its scalar loads and an exit) — unless
    ``scheduler_metadata`` is given.
    ``scheduler_metadata`` (keyword-only, FlashAttention-3's; tfa_fwd_kvcache_varlen_sched): the tensor ``get_scheduler_metadata`` returned for this step's
    ``cu_seqlens_q``, ``max_seqlen_q``, total_q, head counts, ``causal`` and ``pack_gqa`` — the list of the batch's non-empty work items, built once per step on
    the device and reused by every layer.  The launch then carries heads * bound work items (bound: the host-known limit of the list) instead of
    B * heads * ceil(max_seqlen_q * G' / 128); ``out`` and ``lse`` are bit for bit those of the call without it.  The kernel verifies every entry against
    ``cu_seqlens_q``: a list that does not belong to the batch gives unspecified or unwritten rows and never an access outside the tensors.  Refused before any
    launch: given without ``cu_seqlens_q`` (ValueError), a non-tensor (TypeError), not int32 / not on q's device / not contiguous, or a ``numel`` other than
    tfa_kvcache_varlen_schedule_size for this call (ValueError).  None (the default): the call is exactly what it was.
    ``sliding_window`` (keyword-only; tfa_fwd_kvcache_window): the model configs' sliding window over the cache — a host integer w >= 1, the row's own key included,
    with ``causal=True`` required.  Key j is visible to row t of sequence b iff t + shift_b - (w - 1) <= j <= t + shift_b and 0 <= j < len_b, shift_b = len_b - nq_b
    with len_b and nq_b clamped as above (Nq in the 4-D form): FlashAttention's ``window_size=(w - 1, 0)``.  A row that sees no key gives out = 0, lse = +inf.  With
    lo_b = max(0, shift_b - (w - 1)) and lo64_b = lo_b & ~63, the chunks of ``num_splits`` are cut from [lo64_b, len_b), and the kernel loads no block-table entry of a
    page that ends at or before lo64_b and no K/V byte in front of key lo64_b — an engine may free those pages; their table entries may hold anything.  The keys
    from lo64_b on must stay finite (a visited tile's keys left of a row's window are masked; P = 0 times a NaN V row is NaN).  Both layouts, ``scheduler_metadata``
    (``get_scheduler_metadata`` does not learn about the window), paged / contiguous / fp8 caches, ``pack_gqa``, ``k`` / ``v`` appended first, no host
    synchronisation and graph capture: as without it; at Nq == 1 the default and ``pack_gqa=True`` still stream K / V once per K/V head.  ``num_splits=0`` asks
    tfa_fwd_kvcache_window_suggest_splits (the window's reach stands in for the lengths).  With w - 1 >= the capacity the window reaches every key a row can see and the
    call is the plain causal one, through its entry points.  None (the default): the call is exactly what it was.  Refused before any launch: a tensor or
    non-integer (TypeError), w < 1 (ValueError), ``causal=False`` (ValueError).
    ``tree_mask`` (keyword-only; tfa_fwd_kvcache_tree): the verification step of a speculative token tree (EAGLE, Medusa, SpecInfer-style drafts), with
    ``causal=True`` required.  With base_b = len_b - nq_b (len_b and nq_b clamped as above, Nq in the 4-D form; the step's new keys are [base_b, len_b)), key j
    is visible to row t of sequence b iff 0 <= j < len_b, j <= t + base_b (the causal rule as it stands: trees are stored parents-first) and, with s = j - base_b:
    s < 0, or s >= 64, or bit s of ``tree_mask[b, t]`` is set.  The mask only removes keys from what ``causal`` admits, and only among the first 64 new keys of a
    sequence; every row sees the whole committed prefix.  Any sub-causal pattern is legal — it need not be closed under ancestry, a row's own bit may be clear; a
    row that sees no key gives out = 0, lse = +inf; an all-ones word (-1) is plain causal attention for that row, bit for bit.  4-D form: an int64 device tensor
    (B, Nq) with any strides, or a ``torch.bool`` tensor (B, Nq, Nq), True = row t sees new key s, packed into the int64 form by elementwise device ops (no host
    read); Nq <= 64.  Packed form (``cu_seqlens_q``): int64 (total_q,), one word per packed row; a sequence that brings more than 64 rows sees its new keys from
    the 64th on causally (all-ones words on its rows: a chunked-prefill sequence beside tree-verify sequences).  The words are read on the device only: no
    synchronisation, and a captured step replayed after the mask, the lengths and ``cu_seqlens_q`` were overwritten in place computes with the new values.  Masked
    new keys are multiplied by P = 0 and must be finite (they were just appended).  Both layouts, ``scheduler_metadata`` (``get_scheduler_metadata`` does not learn
    about the mask), paged / contiguous / fp8 caches, ``pack_gqa`` (at Nq == 1 the default and True run position-major packed rows), ``k`` / ``v`` appended first,
    every ``num_splits`` (0 asks tfa_fwd_kvcache_tree_suggest_splits: the underlying form's rule — the mask removes no tile), ``return_softmax_lse``: as without it.
    None (the default): the call is exactly what it was.  Refused before any launch: a non-tensor (TypeError); a dtype other than int64 / bool, a wrong shape or
    device, Nq > 64 in the 4-D form, a bool mask in the packed form, ``causal=False``, ``tree_mask`` together with ``sliding_window`` (ValueError).
    Not implemented (refused by name before any launch): rotary_cos / rotary_sin, cache_batch_idx, cache_leftpad, window_size (``sliding_window`` is this call's
    window), softcap, alibi_slopes, fp32 inputs, head dims above 128, float8_e5m2 / float8_e4m3fnuz caches, an fp8 q / k / v."""
    name = "flash_attn_with_kvcache"
    for arg, val in (("rotary_cos", rotary_cos), ("rotary_sin", rotary_sin), ("cache_batch_idx", cache_batch_idx), ("cache_leftpad", cache_leftpad),
                     ("alibi_slopes", alibi_slopes)):
        if val is not None:
            raise NotImplementedError(f"{name}: {arg} is not implemented in the K/V-cache path")
    if tuple(int(w) for w in window_size) != (-1, -1):
        raise NotImplementedError(f"{name}: window_size is not implemented in the K/V-cache path (got {tuple(window_size)}); the window over a cache is "
                                  f"sliding_window=w (w tokens, the row's own included: window_size=(w - 1, 0)) with causal=True")
    if sliding_window is not None:
        if isinstance(sliding_window, (bool, torch.Tensor)) or not isinstance(sliding_window, int):
            raise TypeError(f"{name}: sliding_window must be a host int (got {type(sliding_window).__name__})")
        if sliding_window < 1:
            raise ValueError(f"{name}: sliding_window must be >= 1 (w tokens, the row's own included; got {sliding_window})")
        if not causal:
            raise ValueError(f"{name}: sliding_window needs causal=True (a window without causal is not implemented)")
    if tree_mask is not None:
        if not isinstance(tree_mask, torch.Tensor):
            raise TypeError(f"{name}: tree_mask must be a tensor (got {type(tree_mask).__name__})")
        if not causal:
            raise ValueError(f"{name}: tree_mask needs causal=True (the mask removes keys from what causal admits)")
        if sliding_window is not None:
            raise ValueError(f"{name}: tree_mask together with sliding_window is not implemented")
    if isinstance(softcap, torch.Tensor) or float(softcap) != 0.0:
        raise NotImplementedError(f"{name}: softcap is not implemented in the K/V-cache path")
    if cu_seqlens_q is None and max_seqlen_q is not None:
        raise ValueError(f"{name}: max_seqlen_q belongs to cu_seqlens_q (packed (total_q, H, D) query rows), which was not given")
    if cu_seqlens_q is None and scheduler_metadata is not None:
        raise ValueError(f"{name}: scheduler_metadata belongs to cu_seqlens_q (packed (total_q, H, D) query rows), which was not given")
    if cu_seqlens_q is not None:
        return _flash_attn_with_kvcache_varlen_q(q, k_cache, v_cache, k, v, cache_seqlens, block_table, softmax_scale, causal, num_splits, return_softmax_lse,
                                                 pack_gqa, k_descale, v_descale, cu_seqlens_q, max_seqlen_q, scheduler_metadata, sliding_window, tree_mask)
    for n, t in (("q", q), ("k_cache", k_cache), ("v_cache", v_cache)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError(f"{name}: {n} must be a 4-D tensor")
        if not t.is_cuda:
            raise RuntimeError(f"{n} must be a CUDA tensor")
    B, Nq, H, D = q.shape
    fp8, Hk, capacity, cache_seqlens, num_splits = _kvcache_checks(name, q, k_cache, v_cache, k, v, cache_seqlens, block_table, num_splits, pack_gqa, k_descale,
                                                                   v_descale, B, H, D, False)
    if softmax_scale is None:
        softmax_scale = 1.0 / math.sqrt(D)
    tree = _tree_words(name, tree_mask, q.device, B, Nq) if tree_mask is not None else None

    L = _lib.lib()
    lse = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device) if return_softmax_lse else None
    dense = torch.empty((B, H, Nq, D), dtype=q.dtype, device=q.device)            # what the merge writes; one chunk: the kernel writes it the same way
    p = C.byref(_kvcache_params(q, k_cache, v_cache, dense, lse, cache_seqlens, block_table, k, v, softmax_scale, causal))
    q8 = _kvcache_fp8_arg(fp8, k_descale, v_descale)
    pack = None if pack_gqa is None else (_lib.TFA_PACK_GQA_ON if pack_gqa else _lib.TFA_PACK_GQA_OFF)   # None: the entry points without the argument
    left = _window_left(sliding_window, capacity)
    if left is not None or tree is not None:
        _kvcache_rider_launch(L, p, None, q8, _lib.TFA_PACK_GQA_AUTO if pack is None else pack, left, tree, num_splits, None, q.device)
    elif pack is not None:
        _kvcache_launch(lambda: L.tfa_fwd_kvcache_pack_suggest_splits(p, pack), lambda s: L.tfa_fwd_kvcache_pack_workspace(p, q8, pack, s),
                        lambda s, ws, stream: L.tfa_fwd_kvcache_pack(p, q8, pack, s, ws, stream), num_splits, q.device)
    elif fp8:
        _kvcache_launch(lambda: L.tfa_fwd_kvcache_suggest_splits(p), lambda s: L.tfa_fwd_kvcache_fp8_workspace(p, q8, s),
                        lambda s, ws, stream: L.tfa_fwd_kvcache_fp8(p, q8, s, ws, stream), num_splits, q.device)
    else:
        _kvcache_launch(lambda: L.tfa_fwd_kvcache_suggest_splits(p), lambda s: L.tfa_fwd_kvcache_workspace(p, s),
                        lambda s, ws, stream: L.tfa_fwd_kvcache(p, s, ws, stream), num_splits, q.device)
    out = dense.transpose(1, 2)
    return (out, lse) if return_softmax_lse else out


def _flash_attn_with_kvcache_varlen_q(q, k_cache, v_cache, k, v, cache_seqlens, block_table, softmax_scale, causal, num_splits, return_softmax_lse, pack_gqa,
                                      k_descale, v_descale, cu_seqlens_q, max_seqlen_q, scheduler_metadata=None, sliding_window=None,
                                      tree_mask=None):
    """``flash_attn_with_kvcache(cu_seqlens_q=, max_seqlen_q=)`` (tfa_fwd_kvcache_varlen; with ``scheduler_metadata`` tfa_fwd_kvcache_varlen_sched): the checks of the
    packed form, then the calls.  Every refusal comes before any launch."""
    name = "flash_attn_with_kvcache"
    if not isinstance(q, torch.Tensor) or q.dim() != 3:
        got = tuple(q.shape) if isinstance(q, torch.Tensor) else type(q).__name__
        raise ValueError(f"{name}: with cu_seqlens_q, q must be packed (total_q, H, D) (got {got}); a 4-D q takes no cu_seqlens_q")
    for n, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError(f"{name}: {n} must be a 4-D tensor")
    for n, t in (("q", q), ("k_cache", k_cache), ("v_cache", v_cache)):
        if not t.is_cuda:
            raise RuntimeError(f"{n} must be a CUDA tensor")
    if k is not None or v is not None:
        raise ValueError(f"{name}: with cu_seqlens_q, k / v must be None — kvcache_append_varlen is the append for packed rows (cache_seqlens then includes them)")
    if max_seqlen_q is None or isinstance(max_seqlen_q, (bool, torch.Tensor)) or not isinstance(max_seqlen_q, int) or max_seqlen_q <= 0:
        raise ValueError(f"{name}: cu_seqlens_q needs max_seqlen_q, a positive host int (it sizes the grid; got {max_seqlen_q!r})")
    if not isinstance(cu_seqlens_q, torch.Tensor) or cu_seqlens_q.dtype != torch.int32 or cu_seqlens_q.dim() != 1 or cu_seqlens_q.numel() < 2:
        raise ValueError(f"{name}: cu_seqlens_q must be a 1-D int32 tensor of B + 1 entries")
    if cu_seqlens_q.device != q.device or not cu_seqlens_q.is_contiguous():
        raise ValueError(f"{name}: cu_seqlens_q must be contiguous and on q's device")
    total_q, H, D = q.shape
    B = cu_seqlens_q.numel() - 1
    fp8, Hk, capacity, cache_seqlens, num_splits = _kvcache_checks(name, q, k_cache, v_cache, k, v, cache_seqlens, block_table, num_splits, pack_gqa, k_descale,
                                                                   v_descale, B, H, D, True)
    if softmax_scale is None:
        softmax_scale = 1.0 / math.sqrt(D)
    if scheduler_metadata is not None:
        if not isinstance(scheduler_metadata, torch.Tensor):
            raise TypeError(f"{name}: scheduler_metadata must be the tensor get_scheduler_metadata returned (got {type(scheduler_metadata).__name__})")
        if scheduler_metadata.dtype != torch.int32 or scheduler_metadata.device != q.device or not scheduler_metadata.is_contiguous():
            raise ValueError(f"{name}: scheduler_metadata must be a contiguous int32 tensor on q's device (got {scheduler_metadata.dtype} on "
                             f"{scheduler_metadata.device})")
    tree = _tree_words(name, tree_mask, q.device, None, total_q) if tree_mask is not None else None

    L = _lib.lib()
    if scheduler_metadata is not None:
        want = _scheduler_metadata_size(name, B, H, Hk, int(max_seqlen_q), total_q, pack_gqa, causal)
        if scheduler_metadata.numel() != want:
            raise ValueError(f"{name}: scheduler_metadata holds {scheduler_metadata.numel()} entries, this call's schedule (B {B}, max_seqlen_q {max_seqlen_q}, "
                             f"total_q {total_q}, H {H}, Hk {Hk}, causal {bool(causal)}, pack_gqa {pack_gqa!r}) holds {want}: it was built for another batch")
    lse = torch.empty((H, total_q), dtype=torch.float32, device=q.device) if return_softmax_lse else None
    dense = torch.empty((H, total_q, D), dtype=q.dtype, device=q.device)          # what the merge writes; one chunk: the kernel writes it the same way
    p = _lib.TfaKvcacheParams()
    p.q, p.out = q.data_ptr(), dense.data_ptr()
    p.lse = lse.data_ptr() if lse is not None else None
    p.k_cache, p.v_cache = k_cache.data_ptr(), v_cache.data_ptr()
    p.cache_seqlens = cache_seqlens.data_ptr()
    p.B, p.H, p.Hk, p.Nq, p.D, p.capacity = B, H, Hk, 0, D, capacity              # (Nq is not looked at)
    if block_table is not None:
        p.block_table = block_table.data_ptr()
        p.block_table_stride = block_table.stride(0)
        p.page_size, p.num_pages = k_cache.shape[1], k_cache.shape[0]
    p.q_stride[0], p.q_stride[1], p.q_stride[2] = 0, q.stride(1), q.stride(0)     # {ignored, head, row}
    p.o_stride[0], p.o_stride[1], p.o_stride[2] = 0, total_q * D, D
    for sname, t in (("k_stride", k_cache), ("v_stride", v_cache)):
        arr = getattr(p, sname)
        arr[0], arr[1], arr[2] = t.stride(0), t.stride(2), t.stride(1)
    p.softmax_scale = float(softmax_scale)
    p.is_causal = 1 if causal else 0
    p.dtype = _DT[q.dtype]
    vq = _lib.TfaKvcacheVarlenQ()
    vq.cu_seqlens_q = cu_seqlens_q.data_ptr()
    vq.max_seqlen_q, vq.total_q = int(max_seqlen_q), total_q
    p, pv = C.byref(p), C.byref(vq)
    q8 = _kvcache_fp8_arg(fp8, k_descale, v_descale)
    pack = _lib.TFA_PACK_GQA_OFF if pack_gqa is False else _lib.TFA_PACK_GQA_ON
    left = _window_left(sliding_window, capacity)
    if left is not None or tree is not None:
        _kvcache_rider_launch(L, p, pv, q8, pack, left, tree, num_splits, scheduler_metadata, q.device)
    elif scheduler_metadata is not None:
        meta = C.c_void_p(scheduler_metadata.data_ptr())
        _kvcache_launch(lambda: L.tfa_fwd_kvcache_varlen_suggest_splits(p, pv, pack), lambda s: L.tfa_fwd_kvcache_varlen_workspace(p, pv, q8, pack, s),
                        lambda s, ws, stream: L.tfa_fwd_kvcache_varlen_sched(p, pv, q8, pack, s, meta, ws, stream), num_splits, q.device)
    else:
        _kvcache_launch(lambda: L.tfa_fwd_kvcache_varlen_suggest_splits(p, pv, pack), lambda s: L.tfa_fwd_kvcache_varlen_workspace(p, pv, q8, pack, s),
                        lambda s, ws, stream: L.tfa_fwd_kvcache_varlen(p, pv, q8, pack, s, ws, stream), num_splits, q.device)
    out = dense.transpose(0, 1)
    return (out, lse) if return_softmax_lse else out


def flash_attn_with_kvcache_cascade(q, k_cache, v_cache, *, cu_seqlens_q, max_seqlen_q, cache_seqlens, block_table, prefix_cu_seqlens_q, prefix_max_seqlen_q,
                                    prefix_seqlens, prefix_block_table, softmax_scale=None, causal=True, num_splits=0, prefix_num_splits=0,
                                    return_softmax_lse=False, pack_gqa=None, scheduler_metadata=None, prefix_scheduler_metadata=None):
    """Shared-prefix (cascade) attention over a paged K/V cache (tfa_fwd_kvcache_cascade): the keys a group of sequences shares — one prompt behind n samples, a
    system prompt behind many requests, the common trunk of a beam — are streamed once per GROUP, each sequence's own keys once per sequence, and the two are
    merged by LSE in fp32 before the one rounding of ``out``.

    ``q`` is packed (total_q, H, D) exactly as ``flash_attn_with_kvcache(cu_seqlens_q=)`` takes it; ``k_cache`` / ``v_cache`` one paged 16-bit pool
    (num_pages, page_size, Hk, D) of q's dtype, page_size a multiple of 64, any page / row / head strides; both tables index this pool.
    Level 1, each sequence's OWN keys — ``cu_seqlens_q`` (B + 1,), ``max_seqlen_q``, ``cache_seqlens`` (B,), ``block_table`` (B, max_blocks): the packed-q call over
    the non-shared keys only.  Sequence b owns the rows [q0_b, q0_b + nq_b) (clamped as there) and attends its own keys [0, ulen_b),
    ulen_b = clamp(cache_seqlens[b], 0, max_blocks * page_size), through ``block_table[b]``; ``cache_seqlens`` counts own keys only and includes this step's rows.
    ``causal``: own key j is visible to row t iff j <= t + (ulen_b - nq_b).
    Level 0, each group's SHARED keys — ``prefix_cu_seqlens_q`` (Gn + 1,), ``prefix_max_seqlen_q``, ``prefix_seqlens`` (Gn,), ``prefix_block_table``
    (Gn, prefix_max_blocks): group g owns the packed rows [pcu[g], pcu[g+1]) (clamped by the same rule with ``prefix_max_seqlen_q``; a group is a run of
    consecutive sequences, so the engine builds this array the way it builds ``cu_seqlens_q``) and EVERY row of it sees EVERY key [0, plen_g),
    plen_g = clamp(prefix_seqlens[g], 0, prefix_max_blocks * page_size), through ``prefix_block_table[g]`` — the caller's contract: the shared keys precede all of
    the step's rows.  ``causal`` does not act on level 0; plen_g need not be a multiple of the page size.
    A row's result is softmax attention over the disjoint union of its group's shared keys and its sequence's visible own keys; ``lse`` is the logsumexp over
    that union.  A row in no group takes no shared keys, a row in no sequence no own keys; a row that sees no key at all gives out = 0, lse = +inf: every row of
    ``out`` (total_q, H, D) — a transposed view of the dense (H, total_q, D) buffer the merge writes — and of ``lse`` (H, total_q) is specified.  Overlapping
    groups, or any other garbage in the six device arrays, give unspecified values in the rows concerned and never an access outside the tensors.
    Nothing is read on the host (no synchronisation; a captured step replayed after the six arrays were overwritten in place computes with the new values); bytes
    behind a length read as zeros; ``pack_gqa`` is a scheduling choice only (None / True pack when Hk < H and H / Hk <= 128); everything runs on the current stream.
    ``num_splits`` / ``prefix_num_splits``: key chunks of level 1 / level 0 (0 = tfa_fwd_kvcache_cascade_suggest_splits, each level's own geometry).
    ``scheduler_metadata``: the list ``get_scheduler_metadata(cu_seqlens_q, max_seqlen_q, total_q, H, Hk, causal=causal, pack_gqa=pack_gqa)`` built for level 1;
    ``prefix_scheduler_metadata``: the list the same function builds from ``prefix_cu_seqlens_q`` / ``prefix_max_seqlen_q`` with ``causal=False``.  Results with
    lists are bit for bit those without.
    What runs: a fill of the workspace's LSE words, the packed-q kernel once per level writing fp32 partials, one merge that skips empty parts.  Not
    differentiable.  Refused by name before any launch: a 4-D q, a contiguous cache (``block_table`` None), mismatched B or Gn between a level's three arrays, an
    index array of the wrong dtype / device / contiguity, a missing or non-positive maximum, negative split counts (ValueError); fp8 pools, a k / v dtype other than
    q's (TypeError); an input that requires grad (RuntimeError); head dims and fp32 as the packed-q call refuses them."""
    name = "flash_attn_with_kvcache_cascade"
    if not isinstance(q, torch.Tensor) or q.dim() != 3:
        got = tuple(q.shape) if isinstance(q, torch.Tensor) else type(q).__name__
        raise ValueError(f"{name}: q must be packed (total_q, H, D) (got {got}); the 4-D layout has no cascade form")
    for n, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError(f"{name}: {n} must be a 4-D paged pool (num_pages, page_size, Hk, D)")
    for n, t in (("q", q), ("k_cache", k_cache), ("v_cache", v_cache)):
        if not t.is_cuda:
            raise RuntimeError(f"{n} must be a CUDA tensor")
    if k_cache.dtype == torch.float8_e4m3fn or v_cache.dtype == torch.float8_e4m3fn:
        raise TypeError(f"{name}: fp8 pools are not implemented (got {k_cache.dtype}, {v_cache.dtype}); k_cache and v_cache must have q's 16-bit dtype")
    if block_table is None or prefix_block_table is None:
        raise ValueError(f"{name}: a paged pool only — block_table and prefix_block_table must be given (a contiguous cache has no cascade form)")
    for n, val in (("max_seqlen_q", max_seqlen_q), ("prefix_max_seqlen_q", prefix_max_seqlen_q)):
        if val is None or isinstance(val, (bool, torch.Tensor)) or not isinstance(val, int) or val <= 0:
            raise ValueError(f"{name}: {n} must be a positive host int (it sizes the grid; got {val!r})")
    for n, t in (("cu_seqlens_q", cu_seqlens_q), ("prefix_cu_seqlens_q", prefix_cu_seqlens_q)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1 or t.numel() < 2:
            raise ValueError(f"{name}: {n} must be a 1-D int32 tensor of at least two entries")
        if t.device != q.device or not t.is_contiguous():
            raise ValueError(f"{name}: {n} must be contiguous and on q's device")
    total_q, H, D = q.shape
    B, Gn = cu_seqlens_q.numel() - 1, prefix_cu_seqlens_q.numel() - 1
    for n, lens, table, rows, what in (("cache_seqlens", cache_seqlens, None, B, "B = cu_seqlens_q.numel() - 1"),
                                       ("prefix_seqlens", prefix_seqlens, prefix_block_table, Gn, "Gn = prefix_cu_seqlens_q.numel() - 1")):
        if (not isinstance(lens, torch.Tensor) or lens.dtype != torch.int32 or tuple(lens.shape) != (rows,) or not lens.is_contiguous()
                or lens.device != q.device):
            raise ValueError(f"{name}: {n} must be a contiguous int32 tensor of shape ({rows},) — {what} — on q's device")
        if table is None:
            continue                                      # (block_table: _kvcache_checks' own check, below)
        if not isinstance(table, torch.Tensor) or table.dtype != torch.int32 or table.dim() != 2 or table.shape[0] != rows or table.shape[1] < 1:
            raise ValueError(f"{name}: prefix_block_table must be an int32 tensor of shape ({rows}, prefix_max_blocks) — {what}")
        if table.device != q.device or table.stride(1) != 1:
            raise ValueError(f"{name}: prefix_block_table must be on q's device with unit stride along prefix_max_blocks")
    prefix_num_splits = int(prefix_num_splits)
    if prefix_num_splits < 0:
        raise ValueError(f"{name}: prefix_num_splits must be >= 0 (0 = automatic; got {prefix_num_splits})")
    _, Hk, capacity, cache_seqlens, num_splits = _kvcache_checks(name, q, k_cache, v_cache, None, None, cache_seqlens, block_table, num_splits, pack_gqa, None,
                                                                 None, B, H, D, True)
    if softmax_scale is None:
        softmax_scale = 1.0 / math.sqrt(D)
    metas = []
    for n, md, b, mq, cz in (("scheduler_metadata", scheduler_metadata, B, max_seqlen_q, causal),
                             ("prefix_scheduler_metadata", prefix_scheduler_metadata, Gn, prefix_max_seqlen_q, False)):
        if md is None:
            metas.append(None)
            continue
        if not isinstance(md, torch.Tensor):
            raise TypeError(f"{name}: {n} must be the tensor get_scheduler_metadata returned (got {type(md).__name__})")
        if md.dtype != torch.int32 or md.device != q.device or not md.is_contiguous():
            raise ValueError(f"{name}: {n} must be a contiguous int32 tensor on q's device (got {md.dtype} on {md.device})")
        want = _scheduler_metadata_size(name, b, H, Hk, int(mq), total_q, pack_gqa, cz)
        if md.numel() != want:
            raise ValueError(f"{name}: {n} holds {md.numel()} entries, this level's schedule ({b} sequences, max_seqlen_q {mq}, total_q {total_q}, H {H}, Hk {Hk}, "
                             f"causal {bool(cz)}, pack_gqa {pack_gqa!r}) holds {want}: it was built for another batch")
        metas.append(C.c_void_p(md.data_ptr()))

    L = _lib.lib()
    lse = torch.empty((H, total_q), dtype=torch.float32, device=q.device) if return_softmax_lse else None
    dense = torch.empty((H, total_q, D), dtype=q.dtype, device=q.device)          # what the merge writes
    p = _lib.TfaKvcacheParams()
    p.q, p.out = q.data_ptr(), dense.data_ptr()
    p.lse = lse.data_ptr() if lse is not None else None
    p.k_cache, p.v_cache = k_cache.data_ptr(), v_cache.data_ptr()
    p.cache_seqlens = cache_seqlens.data_ptr()
    p.B, p.H, p.Hk, p.Nq, p.D, p.capacity = B, H, Hk, 0, D, capacity
    p.block_table = block_table.data_ptr()
    p.block_table_stride = block_table.stride(0)
    p.page_size, p.num_pages = k_cache.shape[1], k_cache.shape[0]
    p.q_stride[0], p.q_stride[1], p.q_stride[2] = 0, q.stride(1), q.stride(0)     # {ignored, head, row}
    p.o_stride[0], p.o_stride[1], p.o_stride[2] = 0, total_q * D, D
    for sname, t in (("k_stride", k_cache), ("v_stride", v_cache)):
        arr = getattr(p, sname)
        arr[0], arr[1], arr[2] = t.stride(0), t.stride(2), t.stride(1)
    p.softmax_scale = float(softmax_scale)
    p.is_causal = 1 if causal else 0
    p.dtype = _DT[q.dtype]
    vq = _lib.TfaKvcacheVarlenQ()
    vq.cu_seqlens_q = cu_seqlens_q.data_ptr()
    vq.max_seqlen_q, vq.total_q = int(max_seqlen_q), total_q
    cs = _lib.TfaKvcacheCascade()
    cs.prefix_cu_seqlens_q, cs.prefix_seqlens = prefix_cu_seqlens_q.data_ptr(), prefix_seqlens.data_ptr()
    cs.prefix_block_table, cs.prefix_block_table_stride = prefix_block_table.data_ptr(), prefix_block_table.stride(0)
    cs.num_groups, cs.prefix_max_blocks, cs.prefix_max_seqlen_q = Gn, prefix_block_table.shape[1], int(prefix_max_seqlen_q)
    p, pv, pc = C.byref(p), C.byref(vq), C.byref(cs)
    pack = _lib.TFA_PACK_GQA_OFF if pack_gqa is False else _lib.TFA_PACK_GQA_ON
    if num_splits == 0 or prefix_num_splits == 0:
        s1, s0 = C.c_int(1), C.c_int(1)
        _lib.check(L.tfa_fwd_kvcache_cascade_suggest_splits(p, pv, pc, pack, C.byref(s1), C.byref(s0)))
        num_splits = num_splits or max(1, s1.value)
        prefix_num_splits = prefix_num_splits or max(1, s0.value)
    need = int(L.tfa_fwd_kvcache_cascade_workspace(p, pv, pc, pack, num_splits, prefix_num_splits))
    if need < 0:
        _lib.check(need)
    ws = torch.empty((need,), dtype=torch.float32, device=q.device)
    with torch.cuda.device(q.device):
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(L.tfa_fwd_kvcache_cascade(p, pv, pc, pack, num_splits, prefix_num_splits, metas[0], metas[1], ws.data_ptr(), C.c_void_p(stream)))
    out = dense.transpose(0, 1)
    return (out, lse) if return_softmax_lse else out


def _window_left(sliding_window, capacity):
    """The ``window_left`` of tfa_fwd_kvcache_window for a checked ``sliding_window``, or None where the plain causal entry points run: no window, or one that
    reaches every key a row can see (w - 1 >= capacity — the host knows it)."""
    if sliding_window is None or sliding_window - 1 >= capacity:
        return None
    return sliding_window - 1


def _tree_words(name, tree_mask, device, B, rows):
    """The int64 visibility words of a checked ``tree_mask``: (B, Nq) with its own strides in the 4-D form (``rows`` = Nq), (total_q,) in the packed form (``B``
    None, ``rows`` = total_q).  A bool (B, Nq, Nq) mask is packed by elementwise ops on its device — word[b, t] = sum_s mask[b, t, s] << s, bit 63 the sign bit."""
    if tree_mask.device != device:
        raise ValueError(f"{name}: tree_mask must be on q's device (got {tree_mask.device})")
    if B is None:
        if tree_mask.dtype == torch.bool:
            raise ValueError(f"{name}: with cu_seqlens_q, tree_mask is the int64 layout (total_q,) — one 64-bit word per packed row; a bool mask belongs to the 4-D form")
        if tree_mask.dtype != torch.int64 or tuple(tree_mask.shape) != (rows,):
            raise ValueError(f"{name}: with cu_seqlens_q, tree_mask must be an int64 tensor of shape ({rows},) (got {tree_mask.dtype} {tuple(tree_mask.shape)})")
        return tree_mask
    if rows > 64:
        raise ValueError(f"{name}: tree_mask covers the first 64 new keys of a sequence: Nq <= 64 in the 4-D form (got {rows})")
    if tree_mask.dtype == torch.bool:
        if tuple(tree_mask.shape) != (B, rows, rows):
            raise ValueError(f"{name}: a bool tree_mask must have shape ({B}, {rows}, {rows}) (got {tuple(tree_mask.shape)})")
        bits = torch.arange(rows, dtype=torch.int64, device=tree_mask.device)
        return torch.bitwise_left_shift(tree_mask.to(torch.int64), bits).sum(dim=-1)
    if tree_mask.dtype != torch.int64 or tuple(tree_mask.shape) != (B, rows):
        raise ValueError(f"{name}: tree_mask must be an int64 tensor of shape ({B}, {rows}) or a bool tensor of shape ({B}, {rows}, {rows}) "
                         f"(got {tree_mask.dtype} {tuple(tree_mask.shape)})")
    return tree_mask


def _kvcache_rider_launch(L, p, pv, q8, pack, left, tree, num_splits, scheduler_metadata, device):
    """The one dispatch to tfa_fwd_kvcache_window — or, with ``tree`` (the int64 words; ``left`` is then None), to tfa_fwd_kvcache_tree, whose arguments are the
    same but for the window — from the 4-D (``pv`` None) and the packed-q forms: ``p``, ``pv`` and ``q8`` are the structs by reference."""
    fam, rider = "tfa_fwd_kvcache_window", left
    if tree is not None:
        pt = _lib.TfaKvcacheTree()
        pt.mask = tree.data_ptr()
        pt.batch_stride, pt.row_stride = (tree.stride(0), tree.stride(1)) if tree.dim() == 2 else (0, tree.stride(0))
        fam, rider = "tfa_fwd_kvcache_tree", C.byref(pt)
    meta = C.c_void_p(scheduler_metadata.data_ptr()) if scheduler_metadata is not None else None
    _kvcache_launch(lambda: getattr(L, fam + "_suggest_splits")(p, pv, pack, rider), lambda s: getattr(L, fam + "_workspace")(p, pv, q8, pack, rider, s),
                    lambda s, ws, stream: getattr(L, fam)(p, pv, q8, pack, rider, s, meta, ws, stream), num_splits, device)


def _scheduler_metadata_size(name, B, H, Hk, max_seqlen_q, total_q, pack_gqa, causal):
    """tfa_kvcache_varlen_schedule_size for a batch: the int32 entries of its work list (of the parameter block only B, H, Hk are read)."""
    p = _lib.TfaKvcacheParams()
    p.B, p.H, p.Hk = B, H, Hk
    vq = _lib.TfaKvcacheVarlenQ()
    vq.max_seqlen_q, vq.total_q = max_seqlen_q, total_q
    pack = _lib.TFA_PACK_GQA_OFF if pack_gqa is False else _lib.TFA_PACK_GQA_ON
    n = int(_lib.lib().tfa_kvcache_varlen_schedule_size(C.byref(p), C.byref(vq), pack, 1 if causal else 0))
    if n < 0:
        _lib.check(n)
    return n


def get_scheduler_metadata(cu_seqlens_q, max_seqlen_q, total_q, num_heads, num_heads_k, *, causal=False, pack_gqa=None, out=None):
    """FlashAttention-3's ``get_scheduler_metadata`` for ``flash_attn_with_kvcache(cu_seqlens_q=, max_seqlen_q=, scheduler_metadata=)``
    (tfa_kvcache_varlen_schedule): the work list of a unified batch, built on the device in ONE launch on the current stream — nothing is read on the host, so
    the call does not synchronise and captures into a graph.  Build it once per step and hand it to every layer's attention call.

    ``cu_seqlens_q``: contiguous int32 device tensor of B + 1 entries; ``max_seqlen_q``, ``total_q`` (= q.shape[0]), ``num_heads``, ``num_heads_k``: positive
    host ints; ``causal`` and ``pack_gqa`` as the attention call will get them (None / True pack when Hk < H and H / Hk <= 128).  ``out``: an int32 tensor of
    the right size from an earlier step, overwritten and returned — a captured step keeps one buffer.  Returns the int32 tensor
    (8 + 2 * bound entries: a header — n_items, B, G', causal, max_seqlen_q, total_q, bound, 0 — then one (sequence, item) row per non-empty work item)."""
    name = "get_scheduler_metadata"
    if not isinstance(cu_seqlens_q, torch.Tensor) or cu_seqlens_q.dtype != torch.int32 or cu_seqlens_q.dim() != 1 or cu_seqlens_q.numel() < 2:
        raise ValueError(f"{name}: cu_seqlens_q must be a 1-D int32 tensor of B + 1 entries")
    if not cu_seqlens_q.is_cuda:
        raise RuntimeError("cu_seqlens_q must be a CUDA tensor")
    if not cu_seqlens_q.is_contiguous():
        raise ValueError(f"{name}: cu_seqlens_q must be contiguous")
    for n, val in (("max_seqlen_q", max_seqlen_q), ("total_q", total_q), ("num_heads", num_heads), ("num_heads_k", num_heads_k)):
        if isinstance(val, (bool, torch.Tensor)) or not isinstance(val, int) or val <= 0:
            raise ValueError(f"{name}: {n} must be a positive host int (got {val!r})")
    if num_heads % num_heads_k != 0:
        raise ValueError(f"{name}: the K/V heads ({num_heads_k}) must divide the query heads ({num_heads})")
    if pack_gqa is not None and pack_gqa is not True and pack_gqa is not False:
        raise TypeError(f"{name}: pack_gqa must be None, True or False (got {pack_gqa!r})")
    B = cu_seqlens_q.numel() - 1
    want = _scheduler_metadata_size(name, B, num_heads, num_heads_k, max_seqlen_q, total_q, pack_gqa, causal)
    if out is None:
        out = torch.empty((want,), dtype=torch.int32, device=cu_seqlens_q.device)
    elif not isinstance(out, torch.Tensor):
        raise TypeError(f"{name}: out must be a tensor (got {type(out).__name__})")
    elif out.dtype != torch.int32 or out.device != cu_seqlens_q.device or not out.is_contiguous() or out.numel() != want:
        raise ValueError(f"{name}: out must be a contiguous int32 tensor of {want} entries on cu_seqlens_q's device")
    L = _lib.lib()
    p = _lib.TfaKvcacheParams()
    p.B, p.H, p.Hk = B, num_heads, num_heads_k
    vq = _lib.TfaKvcacheVarlenQ()
    vq.cu_seqlens_q = cu_seqlens_q.data_ptr()
    vq.max_seqlen_q, vq.total_q = max_seqlen_q, total_q
    pack = _lib.TFA_PACK_GQA_OFF if pack_gqa is False else _lib.TFA_PACK_GQA_ON
    with torch.cuda.device(cu_seqlens_q.device):
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(L.tfa_kvcache_varlen_schedule(C.byref(p), C.byref(vq), pack, 1 if causal else 0, C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
    return out


# ---- the serving step's parts around attention: rotary embedding and the packed append (tfa_rotary, tfa_kvcache_append_varlen) ------------------------------
def _rotary_tables(name, cos, sin, dtype, D, device, cos_name="cos", sin_name="sin"):
    """Checks of a (seqlen_ro, rotary_dim / 2) table pair against a tensor of `dtype` and head dim D; returns the pair with 16-byte aligned rows and bases
    (made contiguous once if a row stride or base misses that) and rotary_dim, seqlen_ro."""
    for n, t in ((cos_name, cos), (sin_name, sin)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: {n} must be a tensor (got {type(t).__name__})")
    if cos.dim() != 2 or sin.dim() != 2:
        raise ValueError(f"{name}: {cos_name} / {sin_name} must be 2-D (seqlen_ro, rotary_dim / 2) (got {tuple(cos.shape)}, {tuple(sin.shape)})")
    if cos.shape != sin.shape or cos.dtype != sin.dtype:
        raise ValueError(f"{name}: {cos_name} and {sin_name} must have one shape and dtype (got {tuple(cos.shape)} {cos.dtype}, {tuple(sin.shape)} {sin.dtype})")
    if cos.dtype != dtype and cos.dtype != torch.float32:
        raise ValueError(f"{name}: {cos_name} / {sin_name} must have x's dtype {dtype} or float32 (got {cos.dtype})")
    if cos.device != device or sin.device != device:
        raise ValueError(f"{name}: {cos_name} / {sin_name} must be on x's device")
    seqlen_ro, rotary_dim = cos.shape[0], 2 * cos.shape[1]
    if rotary_dim % 16 != 0 or rotary_dim < 16:
        raise ValueError(f"{name}: rotary_dim must be a positive multiple of 16 (got {rotary_dim})")
    if rotary_dim > D:
        raise ValueError(f"{name}: rotary_dim must not exceed the head dim {D} (got {rotary_dim})")
    if seqlen_ro < 1:
        raise ValueError(f"{name}: {cos_name} / {sin_name} hold no position")
    fixed = []
    for t in (cos, sin):
        if t.stride(1) != 1 or (t.stride(0) * t.element_size()) % 16 != 0 or t.data_ptr() % 16 != 0:
            t = t.contiguous()
        fixed.append(t)
    return fixed[0], fixed[1], rotary_dim, seqlen_ro


def _int32_vector(name, what, t, n, device):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (n,) or not t.is_contiguous() or t.device != device:
        raise ValueError(f"{name}: {what} must be a contiguous int32 tensor of shape ({n},) on x's device")


def _check_rotary_x(name, n, x, cu_seqlens):
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name}: {n} must be a tensor (got {type(x).__name__})")
    if x.dtype not in _DT:
        raise TypeError(f"{name}: float16 or bfloat16 only (got {x.dtype} for {n}; no fp32 / fp8 rotary path)")
    want = 3 if cu_seqlens is not None else 4
    if x.dim() != want:
        raise ValueError(f"{name}: {n} must be " + ("3-D (total, H, D) with cu_seqlens" if want == 3 else "4-D (B, N, H, D) (packed (total, H, D) takes cu_seqlens)")
                         + f" (got {tuple(x.shape)})")
    if not x.is_cuda:
        raise RuntimeError(f"{n} must be a CUDA tensor")
    D = x.shape[-1]
    if D % 8 != 0 or D < 8:
        raise ValueError(f"{name}: the head dim must be a multiple of 8 (got {D})")
    if x.stride(-1) != 1 or any(s % 8 != 0 for s in x.stride()[:-1]):
        raise ValueError(f"{name}: {n} must have unit stride along the head dim and 16-byte aligned rows (strides multiples of 8 elements; got {x.stride()})")
    if min(x.shape) < 1:
        raise ValueError(f"{name}: {n} is empty (got {tuple(x.shape)})")


def _rotary_params(name, xs, outs, cos, sin, interleaved, conjugate, seqlen_offsets, cu_seqlens):
    """A TfaRotaryParams for one or two (x, out) pairs that passed _check_rotary_x; checks the tables, the offsets and cu_seqlens."""
    x = xs[0]
    D = x.shape[-1]
    cos, sin, rotary_dim, seqlen_ro = _rotary_tables(name, cos, sin, x.dtype, D, x.device)
    if cu_seqlens is not None:
        if not isinstance(cu_seqlens, torch.Tensor) or cu_seqlens.dtype != torch.int32 or cu_seqlens.dim() != 1 or cu_seqlens.shape[0] < 2 \
                or not cu_seqlens.is_contiguous() or cu_seqlens.device != x.device:
            raise ValueError(f"{name}: cu_seqlens must be a contiguous int32 tensor of B + 1 entries on x's device")
        B, N = cu_seqlens.shape[0] - 1, x.shape[0]
    else:
        B, N = x.shape[0], x.shape[1]
    p = _lib.TfaRotaryParams()
    if isinstance(seqlen_offsets, torch.Tensor):
        _int32_vector(name, "seqlen_offsets", seqlen_offsets, B, x.device)
        p.seqlen_offsets = seqlen_offsets.data_ptr()
    elif isinstance(seqlen_offsets, int) and not isinstance(seqlen_offsets, bool) and -2 ** 31 <= seqlen_offsets < 2 ** 31:
        p.seqlen_offsets, p.seqlen_offset = None, seqlen_offsets
    else:
        raise ValueError(f"{name}: seqlen_offsets must be a host int or a contiguous int32 tensor of shape ({B},) on x's device")
    p.x, p.out = x.data_ptr(), outs[0].data_ptr()
    p.cos, p.sin = cos.data_ptr(), sin.data_ptr()
    p.cu_seqlens = cu_seqlens.data_ptr() if cu_seqlens is not None else None
    p.B, p.N, p.H, p.D, p.rotary_dim, p.seqlen_ro = B, N, x.shape[-2], D, rotary_dim, seqlen_ro
    p.cos_stride, p.sin_stride = cos.stride(0), sin.stride(0)
    pairs = [("x_stride", x), ("o_stride", outs[0])]
    if len(xs) == 2:
        p.x2, p.out2, p.H2 = xs[1].data_ptr(), outs[1].data_ptr(), xs[1].shape[-2]
        pairs += [("x2_stride", xs[1]), ("o2_stride", outs[1])]
    for field, t in pairs:
        arr = getattr(p, field)
        if cu_seqlens is not None:
            arr[0], arr[1], arr[2] = 0, t.stride(1), t.stride(0)                 # (total, H, D): head, row
        else:
            arr[0], arr[1], arr[2] = t.stride(0), t.stride(2), t.stride(1)      # (B, N, H, D): batch, head, row
    p.dtype = _DT[x.dtype]
    p.cs_dtype = _lib.TFA_F32 if cos.dtype == torch.float32 else p.dtype
    p.interleaved, p.conjugate = (1 if interleaved else 0), (1 if conjugate else 0)
    return p, (cos, sin)


def _rotary_launch(p, device):
    with torch.cuda.device(device):
        _lib.check(_lib.lib().tfa_rotary(C.byref(p), C.c_void_p(torch.cuda.current_stream().cuda_stream)))


class _ApplyRotaryEmb(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cos, sin, interleaved, inplace, seqlen_offsets, cu_seqlens):
        out = x if inplace else torch.empty(x.shape, dtype=x.dtype, device=x.device)
        p, keep = _rotary_params("apply_rotary_emb", (x,), (out,), cos, sin, interleaved, False, seqlen_offsets, cu_seqlens)
        _rotary_launch(p, x.device)
        tensors = [keep[0], keep[1]]
        ctx.has_cu, ctx.offsets = cu_seqlens is not None, seqlen_offsets
        if cu_seqlens is not None:
            tensors.append(cu_seqlens)
        if isinstance(seqlen_offsets, torch.Tensor):
            tensors.append(seqlen_offsets)
            ctx.offsets = None
        ctx.save_for_backward(*tensors)
        ctx.interleaved = interleaved
        if inplace:
            ctx.mark_dirty(x)
        return out

    @staticmethod
    @_once_differentiable
    def backward(ctx, dout):
        saved = list(ctx.saved_tensors)
        cos, sin = saved[0], saved[1]
        cu = saved[2] if ctx.has_cu else None
        offsets = ctx.offsets if ctx.offsets is not None else saved[-1]
        # the conjugate rotation of the incoming gradient.  In place only on a buffer this function owns — the copy it had to make of a gradient whose layout the
        # kernel does not take; a gradient autograd hands over may be shared with other consumers and is read, never written
        if dout.stride(-1) != 1 or any(s % 8 != 0 for s in dout.stride()[:-1]) or dout.data_ptr() % 16 != 0:
            dout = dout.contiguous() if not dout.is_contiguous() else dout.clone()
            dx = dout
        else:
            dx = torch.empty(dout.shape, dtype=dout.dtype, device=dout.device)
        p, _ = _rotary_params("apply_rotary_emb (backward)", (dout,), (dx,), cos, sin, ctx.interleaved, True, offsets, cu)
        _rotary_launch(p, dout.device)
        return dx, None, None, None, None, None, None


def apply_rotary_emb(x, cos, sin, interleaved=False, inplace=False, seqlen_offsets=0, cu_seqlens=None, max_seqlen=None):
    """FlashAttention-2's ``apply_rotary_emb`` as a HIP kernel (tfa_rotary): rotary position embedding of ``x``.

    ``x`` (B, N, H, D), or packed (total, H, D) with ``cu_seqlens`` (int32, B + 1 entries, on the device); float16 / bfloat16, any strides with unit stride along D and
    16-byte aligned rows — ``qkv[:, :, 0]`` of a packed projection works without a copy.  ``cos`` / ``sin`` (seqlen_ro, rotary_dim / 2) of x's dtype or float32,
    rotary_dim a multiple of 16 and at most D, D a multiple of 8.  ``seqlen_offsets``: a host int or an int32 device tensor (B,) — ``cache_seqlens`` is the intended
    argument; row t of sequence b is rotated at position ``seqlen_offsets[b] + t``.  Nothing is read on the host: the call does not synchronise and replays
    correctly in a captured graph after the offsets were overwritten in place.  ``max_seqlen`` is accepted for signature compatibility and not needed.
    fp32 arithmetic, one rounding per output element; pairs (i, i + rotary_dim / 2) (GPT-NeoX) or (2i, 2i + 1) with ``interleaved`` (GPT-J); elements behind
    rotary_dim are copied, and so — bit for bit — are rows whose position lies outside [0, seqlen_ro) and packed rows that belong to no sequence.
    ``inplace=True`` writes into x and returns it.  Differentiable in x (the backward is the conjugate rotation of the incoming gradient; cos, sin and the offsets
    get no gradient)."""
    name = "apply_rotary_emb"
    _check_rotary_x(name, "x", x, cu_seqlens)
    return _ApplyRotaryEmb.apply(x, cos, sin, bool(interleaved), bool(inplace), seqlen_offsets, cu_seqlens)


def apply_rotary_emb_qk_(q, k, cos, sin, interleaved=False, seqlen_offsets=0, cu_seqlens=None):
    """``apply_rotary_emb`` of q and k IN PLACE in ONE launch (tfa_rotary with its second tensor): q (B, N, H, D) and k (B, N, Hk, D) — or packed (total, H, D) /
    (total, Hk, D) with ``cu_seqlens`` — rotated at the same positions, the bits two ``apply_rotary_emb(..., inplace=True)`` calls leave.  Returns (q, k).
    Inference only: an input that requires grad raises."""
    name = "apply_rotary_emb_qk_"
    _check_rotary_x(name, "q", q, cu_seqlens)
    _check_rotary_x(name, "k", k, cu_seqlens)
    if k.dtype != q.dtype or k.device != q.device:
        raise ValueError(f"{name}: q and k must share one dtype and device (got {q.dtype} on {q.device}, {k.dtype} on {k.device})")
    if k.shape[:-2] != q.shape[:-2] or k.shape[-1] != q.shape[-1]:
        raise ValueError(f"{name}: q and k must agree in everything but the head count (got {tuple(q.shape)}, {tuple(k.shape)})")
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad):
        raise RuntimeError(f"{name} is inference-only: an input requires grad (use apply_rotary_emb, or run it under torch.no_grad())")
    p, _ = _rotary_params(name, (q, k), (q, k), cos, sin, interleaved, False, seqlen_offsets, cu_seqlens)
    _rotary_launch(p, q.device)
    return q, k


def _append_varlen_params(k, v, k_cache, v_cache, cu_seqlens, cache_seqlens, block_table, rotary_cos, rotary_sin, rotary_interleaved):
    """A TfaKvcacheAppendVarlenParams for checked arguments: k / v (total, Hk, D), the caches (B | num_pages, rows, Hk, D), tables with aligned rows or None."""
    total, Hk, D = k.shape
    B = cu_seqlens.shape[0] - 1
    capacity = block_table.shape[1] * k_cache.shape[1] if block_table is not None else k_cache.shape[1]
    p = _lib.TfaKvcacheAppendVarlenParams()
    p.k, p.v, p.k_cache, p.v_cache = k.data_ptr(), v.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr()
    p.cu_seqlens, p.cache_seqlens = cu_seqlens.data_ptr(), cache_seqlens.data_ptr()
    p.B, p.total_new, p.Hk, p.D, p.capacity = B, total, Hk, D, capacity
    if block_table is not None:
        p.block_table, p.block_table_stride = block_table.data_ptr(), block_table.stride(0)
        p.page_size, p.num_pages = k_cache.shape[1], k_cache.shape[0]
    else:
        p.block_table = None
    for field, t in (("k_stride", k), ("v_stride", v)):
        arr = getattr(p, field)
        arr[0], arr[1] = t.stride(1), t.stride(0)                               # (total, Hk, D): head, row
    for field, t in (("kc_stride", k_cache), ("vc_stride", v_cache)):
        arr = getattr(p, field)
        arr[0], arr[1], arr[2] = t.stride(0), t.stride(2), t.stride(1)          # (B | pages, rows, Hk, D): batch / page, head, row
    p.dtype = _DT[k.dtype]
    if rotary_cos is not None:
        p.rotary_cos, p.rotary_sin = rotary_cos.data_ptr(), rotary_sin.data_ptr()
        p.cos_stride, p.sin_stride = rotary_cos.stride(0), rotary_sin.stride(0)
        p.rotary_dim, p.seqlen_ro = 2 * rotary_cos.shape[1], rotary_cos.shape[0]
        p.rotary_interleaved = 1 if rotary_interleaved else 0
        p.cs_dtype = _lib.TFA_F32 if rotary_cos.dtype == torch.float32 else p.dtype
    return p


def kvcache_append_varlen(k, v, k_cache, v_cache, cu_seqlens, cache_seqlens, block_table=None, *, rotary_cos=None, rotary_sin=None, rotary_interleaved=False,
                          q=None, k_descale=None, v_descale=None):
    """A unified batch's new K/V rows into a paged or contiguous cache (tfa_kvcache_append_varlen) — the append ``flash_attn_varlen_func(..., block_table=)`` needs.

    ``k`` / ``v`` (total_new, Hk, D) packed, of the caches' 16-bit dtype, any strides with unit stride along D; ``cu_seqlens`` (B + 1,) and ``cache_seqlens`` (B,)
    int32 on the device: sequence b owns rows [cu[b], cu[b+1]) and its row t goes to key position ``cache_seqlens[b] + t``.  The caches: paged
    (num_pages, page_size, Hk, D) with ``block_table`` (B, max_blocks) int32 (page_size a multiple of 64), or contiguous (B, capacity, Hk, D).  Dropped: a position
    below 0 or at / beyond the capacity, a row whose block-table entry is not a page of the pool, a packed row outside every sequence; nothing is stored outside
    the caches.  ``cache_seqlens`` is not advanced.  Nothing is read on the host: no synchronisation, capturable in a graph.
    ``rotary_cos`` / ``rotary_sin``: K is rotated at its key position on the way in (V is copied) — the bits ``apply_rotary_emb(k, cos, sin, cu_seqlens=cu_seqlens,
    seqlen_offsets=cache_seqlens)`` followed by the plain append leaves; the query side is ``q=`` below, or ``apply_rotary_emb(q, ..., cu_seqlens=cu_q,
    seqlen_offsets=cache_seqlens)``.
    ``q`` (needs the tables; tfa_kvcache_append_varlen_ex): packed (total_new, H, D) of k's dtype, any row and head strides with unit stride along D and 16-byte
    aligned rows — ``qkv[:, :H]`` of a packed projection works — rotated IN PLACE in the same launch at the positions K is rotated at, row t of sequence b at
    ``cache_seqlens[b] + t``: the bits ``apply_rotary_emb(q, cos, sin, interleaved, inplace=True, seqlen_offsets=cache_seqlens, cu_seqlens=cu_seqlens)`` leaves.
    Untouched bit for bit: elements behind rotary_dim, rows outside every sequence, rows whose position lies outside [0, seqlen_ro).  q has no capacity: a row
    whose K is dropped still has its q rotated.  No relation between H and Hk is needed.  Precondition: q must not overlap k, v or the caches.
    fp8 caches (tfa_kvcache_append_varlen_ex): ``k_cache`` / ``v_cache`` of dtype ``torch.float8_e4m3fn`` (paged or contiguous, strides multiples of 16 bytes, D a
    multiple of 16) with ``k_descale`` / ``v_descale``, float32 device tensors of shape (B, Hk) with any strides, indexed by the sequence (not the page) and
    read on the device only.  Both are required — ``None`` does not mean 1.0 here; unit scales are ``torch.ones(1, 1, device=...).expand(B, Hk)``.  k / v stay
    16-bit; stored byte = ``rne_e4m3fn(clamp(float(x) / descale[b, hk], -448, 448))``, a true fp32 division, NaN stays NaN — the 4-D fp8 append's bytes; with
    tables K is rotated and rounded once to its 16-bit dtype first, then quantised.  Positions, page lookup and drop rules are the 16-bit append's.
    Without ``q`` and descales the call is tfa_kvcache_append_varlen's.  Not differentiable."""
    name = "kvcache_append_varlen"
    for n, t in (("k", k), ("v", v), ("k_cache", k_cache), ("v_cache", v_cache), ("cu_seqlens", cu_seqlens), ("cache_seqlens", cache_seqlens)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: {n} must be a tensor (got {type(t).__name__})")
    if k.dtype not in _DT:
        raise TypeError(f"{name}: float16 or bfloat16 only (got {k.dtype} for k)")
    if v.dtype != k.dtype:
        raise TypeError(f"{name}: v must have k's dtype {k.dtype} (got {v.dtype})")
    fp8s = tuple(getattr(torch, n) for n in ("float8_e4m3fn", "float8_e5m2", "float8_e4m3fnuz", "float8_e5m2fnuz") if hasattr(torch, n))
    fp8 = k_cache.dtype in fp8s or v_cache.dtype in fp8s
    if fp8:
        if k_cache.dtype != v_cache.dtype:
            raise TypeError(f"{name}: k_cache and v_cache must share one dtype (got {k_cache.dtype}, {v_cache.dtype})")
        if k_cache.dtype != torch.float8_e4m3fn:
            raise TypeError(f"{name}: fp8 caches must be torch.float8_e4m3fn (got {k_cache.dtype}; float8_e5m2 and float8_e4m3fnuz caches are not supported)")
        if k_descale is None or v_descale is None:
            raise TypeError(f"{name}: fp8 caches are not served without k_descale / v_descale (both are required; unit scales are "
                            f"torch.ones(1, 1, device=...).expand(B, Hk))")
    else:
        for n, t in (("k_cache", k_cache), ("v_cache", v_cache)):
            if t.dtype != k.dtype:
                raise TypeError(f"{name}: {n} must have k's dtype {k.dtype}, or both caches be torch.float8_e4m3fn with k_descale / v_descale (got {t.dtype})")
        if k_descale is not None or v_descale is not None:
            raise TypeError(f"{name}: k_descale / v_descale belong to torch.float8_e4m3fn caches (got {k_cache.dtype} caches)")
    for n, t in (("k", k), ("v", v)):
        if t.dim() != 3:
            raise ValueError(f"{name}: {n} must be 3-D (total_new, Hk, D) (got {tuple(t.shape)})")
    for n, t in (("k_cache", k_cache), ("v_cache", v_cache)):
        if t.dim() != 4:
            raise ValueError(f"{name}: {n} must be a 4-D tensor (got {tuple(t.shape)})")
    for n, t in (("k", k), ("v", v), ("k_cache", k_cache), ("v_cache", v_cache)):
        if not t.is_cuda:
            raise RuntimeError(f"{n} must be a CUDA tensor")
    total, Hk, D = k.shape
    if k.shape != v.shape or total < 1 or Hk < 1:
        raise ValueError(f"{name}: k and v must have one non-empty shape (got {tuple(k.shape)}, {tuple(v.shape)})")
    if D % 8 != 0 or D < 8 or D > 128:
        raise ValueError(f"{name}: the head dim must be a multiple of 8 up to 128 (got {D})")
    if fp8 and D % 16 != 0:
        raise ValueError(f"{name}: with an fp8 cache the head dim must be a multiple of 16 (got {D})")
    if k_cache.shape != v_cache.shape or k_cache.shape[2] != Hk or k_cache.shape[3] != D:
        raise ValueError(f"{name}: k_cache and v_cache must have one shape (..., {Hk}, {D}) (got {tuple(k_cache.shape)}, {tuple(v_cache.shape)})")
    for n, t in (("k", k), ("v", v), ("k_cache", k_cache), ("v_cache", v_cache)):
        if t.stride(-1) != 1 or any((s * t.element_size()) % 16 != 0 for s in t.stride()[:-1]) or t.device != k.device:
            raise ValueError(f"{name}: {n} must be on k's device with unit stride along the head dim and 16-byte aligned rows (got strides {t.stride()})")
    if cu_seqlens.dtype != torch.int32 or cu_seqlens.dim() != 1 or cu_seqlens.shape[0] < 2 or not cu_seqlens.is_contiguous() or cu_seqlens.device != k.device:
        raise ValueError(f"{name}: cu_seqlens must be a contiguous int32 tensor of B + 1 entries on k's device")
    B = cu_seqlens.shape[0] - 1
    if cache_seqlens.dtype != torch.int32 or tuple(cache_seqlens.shape) != (B,) or not cache_seqlens.is_contiguous() or cache_seqlens.device != k.device:
        raise ValueError(f"{name}: cache_seqlens must be a contiguous int32 tensor of shape ({B},) on k's device")
    if block_table is not None:
        if not isinstance(block_table, torch.Tensor) or block_table.dtype != torch.int32 or block_table.dim() != 2 or block_table.shape[0] != B \
                or block_table.shape[1] < 1:
            raise ValueError(f"{name}: block_table must be an int32 tensor of shape ({B}, max_blocks)")
        if block_table.device != k.device or block_table.stride(1) != 1:
            raise ValueError(f"{name}: block_table must be on k's device with unit stride along max_blocks")
        if k_cache.shape[1] % 64 != 0 or k_cache.shape[1] <= 0 or k_cache.shape[0] < 1:
            raise ValueError(f"{name}: the page size must be a positive multiple of 64 (got {k_cache.shape[1]})")
        capacity = block_table.shape[1] * k_cache.shape[1]
    else:
        if k_cache.shape[0] != B:
            raise ValueError(f"{name}: a contiguous cache must have one slice per sequence ({B}; got {k_cache.shape[0]})")
        capacity = k_cache.shape[1]
    if capacity <= 0 or capacity >= 2 ** 31:
        raise ValueError(f"{name}: the cache must hold between 1 and 2^31 - 1 keys per sequence (got {capacity})")
    if (rotary_cos is None) != (rotary_sin is None):
        raise ValueError(f"{name}: rotary_cos and rotary_sin must be given together")
    if rotary_cos is not None:
        rotary_cos, rotary_sin, rotary_dim, seqlen_ro = _rotary_tables(name, rotary_cos, rotary_sin, k.dtype, D, k.device, "rotary_cos", "rotary_sin")
    if fp8:
        for n, t in (("k_descale", k_descale), ("v_descale", v_descale)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
                raise TypeError(f"{name}: {n} must be a float32 tensor")
            if tuple(t.shape) != (B, Hk) or t.device != k.device:
                raise TypeError(f"{name}: {n} must have shape ({B}, {Hk}) — B = cu_seqlens.numel() - 1 — on k's device (got {tuple(t.shape)} on {t.device})")
    if q is not None:
        if not isinstance(q, torch.Tensor):
            raise TypeError(f"{name}: q must be a tensor (got {type(q).__name__})")
        if q.dtype != k.dtype:
            raise TypeError(f"{name}: q must have k's dtype {k.dtype} (got {q.dtype})")
        if rotary_cos is None:
            raise ValueError(f"{name}: q is rotated by rotary_cos / rotary_sin and needs them")
        if q.dim() != 3 or q.shape[0] != total or q.shape[1] < 1 or q.shape[2] != D:
            raise ValueError(f"{name}: q must be 3-D ({total}, H, {D}) — k's rows and head dim (got {tuple(q.shape)})")
        if q.device != k.device:
            raise ValueError(f"{name}: q must be on k's device (got {q.device})")
        if q.stride(2) != 1 or any(s % 8 != 0 for s in q.stride()[:2]):
            raise ValueError(f"{name}: q must have unit stride along the head dim and 16-byte aligned rows (strides multiples of 8 elements; got {q.stride()})")
        if q.data_ptr() % 16 != 0:
            raise ValueError(f"{name}: q must start at a 16-byte aligned address")
    if torch.is_grad_enabled() and any(t.requires_grad for t in (k, v, k_cache, v_cache) + ((q,) if q is not None else ())):
        raise RuntimeError(f"{name} is not differentiable: an input requires grad (run it under torch.no_grad() or detach the inputs)")

    p = _append_varlen_params(k, v, k_cache, v_cache, cu_seqlens, cache_seqlens, block_table, rotary_cos, rotary_sin, rotary_interleaved)
    if not fp8 and q is None:
        with torch.cuda.device(k.device):
            _lib.check(_lib.lib().tfa_kvcache_append_varlen(C.byref(p), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return None
    p8 = rq = None
    if fp8:
        p8 = _lib.TfaKvcacheFp8()
        p8.format = _lib.TFA_KV_E4M3
        for ptr, strides, t in (("k_descale", p8.k_descale_stride, k_descale), ("v_descale", p8.v_descale_stride, v_descale)):
            setattr(p8, ptr, t.data_ptr())
            strides[0], strides[1] = t.stride(0), t.stride(1)
    if q is not None:
        rq = _lib.TfaAppendQ()
        rq.q, rq.H = q.data_ptr(), q.shape[1]
        rq.q_stride[0], rq.q_stride[1] = q.stride(1), q.stride(0)               # (total, H, D): head, row
    with torch.cuda.device(k.device):
        _lib.check(_lib.lib().tfa_kvcache_append_varlen_ex(C.byref(p), C.byref(p8) if fp8 else None, C.byref(rq) if rq is not None else None,
                                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return None
