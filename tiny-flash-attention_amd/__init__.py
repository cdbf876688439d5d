"""MI355X-native (gfx950) FlashAttention-2 forward — the one hot path of 66RING/tiny-flash-attention.

Host side: a thin Python mirror of the reference's operator interface over the C ABI of
``include/tfa.h`` (``lib/libtfa_hip.so``, hand-written HIP).  PyTorch is used only for device
memory, streams and torch.distributed.

Reference-named entry points (same names, argument order and return shapes):

* ``flash_attention_v2_cutlass(q, k, v, is_causal, softmax_scale) -> [out, lse]``
  (flash_attention_cutlass/csrc/attention_api.cpp:6-10, flash_attention.cu:741-772)
* ``flash_attention_v2_cuda(q, k, v) -> out`` (flash_attention_cuda/csrc/attention_api.cpp:6-14)
* ``flash_attn(q, k, v, is_causal, softmax_scale) -> out`` (flash_attention_c/csrc/ops.cu:4-8)

FlashAttention-2's training interface: ``flash_attn_func`` / ``flash_attn_varlen_func`` with ``causal``, ``window_size``, ``alibi_slopes`` and ``softcap``
(GQA, bottom-right aligned masks, a deterministic backward); ``flash_attn_fwd`` / ``_bwd`` and their ``_varlen`` forms underneath.  ``flash_attn_func`` also
takes ``attn_bias``: a dense additive bias or mask as scaled_dot_product_attention's ``attn_mask`` (fixed-length calls; no gradient for the bias).
Its inference interface: ``flash_attn_with_kvcache`` (device-side ``cache_seqlens``, paged K/V, in-place append; 16-bit or fp8 e4m3 caches with ``k_descale`` / ``v_descale``;
packed ragged query rows with ``cu_seqlens_q``, and ``get_scheduler_metadata`` / ``scheduler_metadata=`` for a work list built once per step on the device) and
``flash_attn_with_kvcache_cascade`` (shared-prefix attention: a group's shared pages streamed once per group, each sequence's own once, one merge).
Around attention: ``apply_rotary_emb`` / ``apply_rotary_emb_qk_`` (rotary embedding at device-side positions) and ``kvcache_append_varlen`` (a unified batch's
new K/V rows into a paged or contiguous cache — 16-bit or e4m3 with descales —, K optionally rotated on the way in and q in place in the same launch) — with the two attention calls a whole decode or chunked-prefill step.
"""
from .ops import (  # noqa: F401
    flash_attention_v2_cutlass,
    flash_attention_v2_cuda,
    flash_attention_v1_cuda,
    self_attention_cuda,
    flash_attn,
    naive_attn,
    flash_attn_func,
    flash_attn_fwd,
    flash_attn_bwd,
    flash_attn_fwd_splitkv,
    merge_partials,
    flash_attn_varlen_func,
    flash_attn_varlen_fwd,
    flash_attn_varlen_bwd,
    flash_attn_with_kvcache,
    flash_attn_with_kvcache_cascade,
    get_scheduler_metadata,
    apply_rotary_emb,
    apply_rotary_emb_qk_,
    kvcache_append_varlen,
)
from . import _lib  # noqa: F401

__all__ = [
    "flash_attention_v2_cutlass",
    "flash_attention_v2_cuda",
    "flash_attention_v1_cuda",
    "self_attention_cuda",
    "flash_attn",
    "naive_attn",
    "flash_attn_func",
    "flash_attn_fwd",
    "flash_attn_bwd",
    "flash_attn_fwd_splitkv",
    "merge_partials",
    "flash_attn_varlen_func",
    "flash_attn_varlen_fwd",
    "flash_attn_varlen_bwd",
    "flash_attn_with_kvcache",
    "flash_attn_with_kvcache_cascade",
    "get_scheduler_metadata",
    "apply_rotary_emb",
    "apply_rotary_emb_qk_",
    "kvcache_append_varlen",
]
