"""ctypes binding of include/tfa.h.  Fails loudly when the HIP library is missing — there is
no CPU or PyTorch fallback on the product path."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TFA_LIB") or os.path.join(_HERE, "lib", "libtfa_hip.so")   # TFA_LIB: developer override (A/B of builds)

TFA_F16, TFA_BF16, TFA_F32 = 0, 1, 2

# every symbol include/tfa.h declares
SYMBOLS = (
    "tfa_version",
    "tfa_debug_mfma_ceiling",
    "tfa_strerror",
    "tfa_fwd",
    "tfa_fwd_bhnd",
    "tfa_fwd_bhnd_f32out",
    "tfa_fwd_plan",
    "tfa_fwd_variant",
    "tfa_fwd_rounding_rule",
    "tfa_fwd_time",
    "tfa_set_variant",
    "tfa_get_variant",
    "tfa_num_variants",
    "tfa_variant_name",
    "tfa_variant_available",
    "tfa_fwd_work",
    "tfa_debug_set_trace",
    "tfa_debug_set_flags",
    "tfa_debug_decode",
    "tfa_merge",
    "tfa_fwd_splitkv",
    "tfa_fwd_splitkv_workspace",
    "tfa_fwd_suggest_splits",
    "tfa_bwd",
    "tfa_bwd_plan",
    "tfa_debug_bwd_split",
    "tfa_bwd_workspace_bytes",
    "tfa_bwd_work",
    "tfa_bwd_time",
    "tfa_fwd_varlen",
    "tfa_fwd_varlen_plan",
    "tfa_fwd_varlen_variant",
    "tfa_fwd_varlen_rounding_rule",
    "tfa_bwd_varlen",
    "tfa_fwd_varlen_paged",
    "tfa_fwd_varlen_paged_plan",
    "tfa_fwd_varlen_paged_variant",
    "tfa_fwd_varlen_paged_rounding_rule",
    "tfa_fwd_local",
    "tfa_fwd_local_plan",
    "tfa_fwd_local_variant",
    "tfa_fwd_local_rounding_rule",
    "tfa_fwd_varlen_local",
    "tfa_fwd_varlen_local_plan",
    "tfa_fwd_varlen_local_variant",
    "tfa_fwd_varlen_local_rounding_rule",
    "tfa_bwd_local",
    "tfa_bwd_local_plan",
    "tfa_bwd_varlen_local",
    "tfa_bwd_varlen_local_plan",
    "tfa_fwd_alibi",
    "tfa_fwd_alibi_plan",
    "tfa_fwd_alibi_variant",
    "tfa_fwd_alibi_rounding_rule",
    "tfa_fwd_varlen_alibi",
    "tfa_fwd_varlen_alibi_plan",
    "tfa_fwd_varlen_alibi_variant",
    "tfa_fwd_varlen_alibi_rounding_rule",
    "tfa_bwd_alibi",
    "tfa_bwd_alibi_plan",
    "tfa_bwd_varlen_alibi",
    "tfa_bwd_varlen_alibi_plan",
    "tfa_fwd_softcap",
    "tfa_fwd_softcap_plan",
    "tfa_fwd_softcap_variant",
    "tfa_fwd_softcap_rounding_rule",
    "tfa_fwd_varlen_softcap",
    "tfa_fwd_varlen_softcap_plan",
    "tfa_fwd_varlen_softcap_variant",
    "tfa_fwd_varlen_softcap_rounding_rule",
    "tfa_bwd_softcap",
    "tfa_bwd_softcap_plan",
    "tfa_bwd_varlen_softcap",
    "tfa_bwd_varlen_softcap_plan",
    "tfa_fwd_bias",
    "tfa_fwd_bias_plan",
    "tfa_fwd_bias_variant",
    "tfa_fwd_bias_rounding_rule",
    "tfa_bwd_bias",
    "tfa_bwd_bias_plan",
    "tfa_fwd_kvcache",
    "tfa_fwd_kvcache_workspace",
    "tfa_fwd_kvcache_plan",
    "tfa_fwd_kvcache_suggest_splits",
    "tfa_kvcache_append",
    "tfa_fwd_kvcache_fp8",
    "tfa_fwd_kvcache_fp8_workspace",
    "tfa_fwd_kvcache_fp8_plan",
    "tfa_kvcache_append_fp8",
    "tfa_fwd_kvcache_pack",
    "tfa_fwd_kvcache_pack_workspace",
    "tfa_fwd_kvcache_pack_plan",
    "tfa_fwd_kvcache_pack_suggest_splits",
    "tfa_fwd_kvcache_varlen",
    "tfa_fwd_kvcache_varlen_workspace",
    "tfa_fwd_kvcache_varlen_plan",
    "tfa_fwd_kvcache_varlen_suggest_splits",
    "tfa_kvcache_varlen_schedule_size",
    "tfa_kvcache_varlen_schedule",
    "tfa_kvcache_varlen_schedule_plan",
    "tfa_fwd_kvcache_varlen_sched",
    "tfa_fwd_kvcache_varlen_sched_plan",
    "tfa_fwd_kvcache_window",
    "tfa_fwd_kvcache_window_plan",
    "tfa_fwd_kvcache_window_workspace",
    "tfa_fwd_kvcache_window_suggest_splits",
    "tfa_fwd_kvcache_tree",
    "tfa_fwd_kvcache_tree_plan",
    "tfa_fwd_kvcache_tree_workspace",
    "tfa_fwd_kvcache_tree_suggest_splits",
    "tfa_fwd_kvcache_cascade",
    "tfa_fwd_kvcache_cascade_workspace",
    "tfa_fwd_kvcache_cascade_plan",
    "tfa_fwd_kvcache_cascade_suggest_splits",
    "tfa_rotary",
    "tfa_rotary_plan",
    "tfa_kvcache_append_varlen",
    "tfa_kvcache_append_varlen_plan",
    "tfa_kvcache_append_varlen_ex",
    "tfa_kvcache_append_varlen_ex_plan",
)


class TfaFwdParams(C.Structure):
    """struct tfa_fwd_params (include/tfa.h)."""

    _fields_ = [
        ("q", C.c_void_p),
        ("k", C.c_void_p),
        ("v", C.c_void_p),
        ("out", C.c_void_p),
        ("lse", C.c_void_p),
        ("B", C.c_int32),
        ("H", C.c_int32),
        ("Hk", C.c_int32),
        ("Nq", C.c_int32),
        ("Nk", C.c_int32),
        ("D", C.c_int32),
        ("q_stride", C.c_int64 * 3),
        ("k_stride", C.c_int64 * 3),
        ("v_stride", C.c_int64 * 3),
        ("o_stride", C.c_int64 * 3),
        ("softmax_scale", C.c_float),
        ("is_causal", C.c_int32),
        ("dtype", C.c_int32),
        ("out_dtype", C.c_int32),
        ("kv_offset", C.c_int64),
        ("nk_total", C.c_int64),
        ("flags", C.c_int32),
        ("reserved_", C.c_int32),
    ]


TFA_FWD_EXACT_MAX = 1   # tfa_fwd_params::flags (include/tfa.h)


class TfaBwdParams(C.Structure):
    """struct tfa_bwd_params (include/tfa.h)."""

    _fields_ = [
        ("q", C.c_void_p),
        ("k", C.c_void_p),
        ("v", C.c_void_p),
        ("out", C.c_void_p),
        ("dout", C.c_void_p),
        ("lse", C.c_void_p),
        ("dq", C.c_void_p),
        ("dk", C.c_void_p),
        ("dv", C.c_void_p),
        ("delta", C.c_void_p),
        ("B", C.c_int32),
        ("H", C.c_int32),
        ("Hk", C.c_int32),
        ("Nq", C.c_int32),
        ("Nk", C.c_int32),
        ("D", C.c_int32),
        ("q_stride", C.c_int64 * 3),
        ("k_stride", C.c_int64 * 3),
        ("v_stride", C.c_int64 * 3),
        ("o_stride", C.c_int64 * 3),
        ("do_stride", C.c_int64 * 3),
        ("dq_stride", C.c_int64 * 3),
        ("dk_stride", C.c_int64 * 3),
        ("dv_stride", C.c_int64 * 3),
        ("softmax_scale", C.c_float),
        ("is_causal", C.c_int32),
        ("dtype", C.c_int32),
        ("grad_dtype", C.c_int32),
        ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_int64),
    ]


class TfaVarlenFwdParams(C.Structure):
    """struct tfa_varlen_fwd_params (include/tfa.h): packed variable-length batches, strides as (head, row) pairs."""

    _fields_ = [
        ("q", C.c_void_p),
        ("k", C.c_void_p),
        ("v", C.c_void_p),
        ("out", C.c_void_p),
        ("lse", C.c_void_p),
        ("cu_seqlens_q", C.c_void_p),
        ("cu_seqlens_k", C.c_void_p),
        ("B", C.c_int32),
        ("H", C.c_int32),
        ("Hk", C.c_int32),
        ("D", C.c_int32),
        ("max_seqlen_q", C.c_int32),
        ("max_seqlen_k", C.c_int32),
        ("total_q", C.c_int32),
        ("total_k", C.c_int32),
        ("q_stride", C.c_int64 * 2),
        ("k_stride", C.c_int64 * 2),
        ("v_stride", C.c_int64 * 2),
        ("o_stride", C.c_int64 * 2),
        ("softmax_scale", C.c_float),
        ("is_causal", C.c_int32),
        ("dtype", C.c_int32),
        ("out_dtype", C.c_int32),
        ("flags", C.c_int32),
        ("reserved_", C.c_int32),
    ]


class TfaPagedKv(C.Structure):
    """struct tfa_paged_kv (include/tfa.h): the page pool and block table of tfa_fwd_varlen_paged, handed over beside TfaVarlenFwdParams."""

    _fields_ = [
        ("block_table", C.c_void_p),
        ("table_stride", C.c_int64),
        ("max_blocks", C.c_int32),
        ("page_size", C.c_int32),
        ("num_pages", C.c_int32),
        ("reserved_", C.c_int32),
        ("k_page_stride", C.c_int64),
        ("v_page_stride", C.c_int64),
    ]


class TfaAttnBias(C.Structure):
    """struct tfa_attn_bias (include/tfa.h): the dense additive bias of tfa_fwd_bias / tfa_bwd_bias, handed over beside TfaFwdParams / TfaBwdParams."""

    _fields_ = [
        ("bias", C.c_void_p),
        ("dtype", C.c_int32),
        ("reserved_", C.c_int32),
        ("stride", C.c_int64 * 3),
    ]


class TfaVarlenBwdParams(C.Structure):
    """struct tfa_varlen_bwd_params (include/tfa.h)."""

    _fields_ = [
        ("q", C.c_void_p),
        ("k", C.c_void_p),
        ("v", C.c_void_p),
        ("out", C.c_void_p),
        ("dout", C.c_void_p),
        ("lse", C.c_void_p),
        ("dq", C.c_void_p),
        ("dk", C.c_void_p),
        ("dv", C.c_void_p),
        ("delta", C.c_void_p),
        ("cu_seqlens_q", C.c_void_p),
        ("cu_seqlens_k", C.c_void_p),
        ("B", C.c_int32),
        ("H", C.c_int32),
        ("Hk", C.c_int32),
        ("D", C.c_int32),
        ("max_seqlen_q", C.c_int32),
        ("max_seqlen_k", C.c_int32),
        ("total_q", C.c_int32),
        ("total_k", C.c_int32),
        ("q_stride", C.c_int64 * 2),
        ("k_stride", C.c_int64 * 2),
        ("v_stride", C.c_int64 * 2),
        ("o_stride", C.c_int64 * 2),
        ("do_stride", C.c_int64 * 2),
        ("dq_stride", C.c_int64 * 2),
        ("dk_stride", C.c_int64 * 2),
        ("dv_stride", C.c_int64 * 2),
        ("softmax_scale", C.c_float),
        ("is_causal", C.c_int32),
        ("dtype", C.c_int32),
        ("grad_dtype", C.c_int32),
        ("flags", C.c_int32),
        ("reserved_", C.c_int32),
    ]


class TfaKvcacheParams(C.Structure):
    """struct tfa_kvcache_params (include/tfa.h): attention over a K/V cache with device-side lengths, contiguous or paged."""

    _fields_ = [
        ("q", C.c_void_p),
        ("out", C.c_void_p),
        ("lse", C.c_void_p),
        ("k_cache", C.c_void_p),
        ("v_cache", C.c_void_p),
        ("block_table", C.c_void_p),
        ("cache_seqlens", C.c_void_p),
        ("k_new", C.c_void_p),
        ("v_new", C.c_void_p),
        ("B", C.c_int32),
        ("H", C.c_int32),
        ("Hk", C.c_int32),
        ("Nq", C.c_int32),
        ("D", C.c_int32),
        ("capacity", C.c_int32),
        ("n_new", C.c_int32),
        ("page_size", C.c_int32),
        ("num_pages", C.c_int32),
        ("reserved_", C.c_int32),
        ("q_stride", C.c_int64 * 3),
        ("o_stride", C.c_int64 * 3),
        ("k_stride", C.c_int64 * 3),
        ("v_stride", C.c_int64 * 3),
        ("knew_stride", C.c_int64 * 3),
        ("vnew_stride", C.c_int64 * 3),
        ("block_table_stride", C.c_int64),
        ("softmax_scale", C.c_float),
        ("is_causal", C.c_int32),
        ("dtype", C.c_int32),
        ("reserved2_", C.c_int32),
    ]


TFA_KV_E4M3 = 1
TFA_PACK_GQA_AUTO, TFA_PACK_GQA_ON, TFA_PACK_GQA_OFF = 0, 1, 2   # tfa_fwd_kvcache_pack's pack_gqa


class TfaKvcacheFp8(C.Structure):
    """struct tfa_kvcache_fp8 (include/tfa.h): the descales of an e4m3 K/V cache, handed to the _fp8 entry points beside TfaKvcacheParams."""

    _fields_ = [
        ("k_descale", C.c_void_p),
        ("v_descale", C.c_void_p),
        ("k_descale_stride", C.c_int64 * 2),
        ("v_descale_stride", C.c_int64 * 2),
        ("format", C.c_int32),
        ("reserved_", C.c_int32),
    ]


class TfaKvcacheTree(C.Structure):
    """struct tfa_kvcache_tree (include/tfa.h): the visibility words of tfa_fwd_kvcache_tree, handed over beside TfaKvcacheParams."""

    _fields_ = [
        ("mask", C.c_void_p),
        ("batch_stride", C.c_int64),
        ("row_stride", C.c_int64),
    ]


class TfaKvcacheCascade(C.Structure):
    """struct tfa_kvcache_cascade (include/tfa.h): the groups' shared keys of tfa_fwd_kvcache_cascade, handed over beside TfaKvcacheParams and TfaKvcacheVarlenQ."""

    _fields_ = [
        ("prefix_cu_seqlens_q", C.c_void_p),
        ("prefix_seqlens", C.c_void_p),
        ("prefix_block_table", C.c_void_p),
        ("prefix_block_table_stride", C.c_int64),
        ("num_groups", C.c_int32),
        ("prefix_max_blocks", C.c_int32),
        ("prefix_max_seqlen_q", C.c_int32),
        ("reserved_", C.c_int32),
    ]


class TfaKvcacheVarlenQ(C.Structure):
    """struct tfa_kvcache_varlen_q (include/tfa.h): the packed query rows of tfa_fwd_kvcache_varlen, handed over beside TfaKvcacheParams."""

    _fields_ = [
        ("cu_seqlens_q", C.c_void_p),
        ("max_seqlen_q", C.c_int32),
        ("total_q", C.c_int32),
        ("reserved_", C.c_int32 * 2),
    ]


class TfaRotaryParams(C.Structure):
    """struct tfa_rotary_params (include/tfa.h): rotary embedding of one tensor, or of two (q and k) in one launch."""

    _fields_ = [
        ("x", C.c_void_p),
        ("out", C.c_void_p),
        ("x2", C.c_void_p),
        ("out2", C.c_void_p),
        ("cos", C.c_void_p),
        ("sin", C.c_void_p),
        ("seqlen_offsets", C.c_void_p),
        ("cu_seqlens", C.c_void_p),
        ("B", C.c_int32),
        ("N", C.c_int32),
        ("H", C.c_int32),
        ("H2", C.c_int32),
        ("D", C.c_int32),
        ("rotary_dim", C.c_int32),
        ("seqlen_ro", C.c_int32),
        ("seqlen_offset", C.c_int32),
        ("x_stride", C.c_int64 * 3),
        ("o_stride", C.c_int64 * 3),
        ("x2_stride", C.c_int64 * 3),
        ("o2_stride", C.c_int64 * 3),
        ("cos_stride", C.c_int64),
        ("sin_stride", C.c_int64),
        ("dtype", C.c_int32),
        ("cs_dtype", C.c_int32),
        ("interleaved", C.c_int32),
        ("conjugate", C.c_int32),
    ]


class TfaKvcacheAppendVarlenParams(C.Structure):
    """struct tfa_kvcache_append_varlen_params (include/tfa.h): packed new K/V rows into a paged or contiguous cache, K optionally rotated on the way in."""

    _fields_ = [
        ("k", C.c_void_p),
        ("v", C.c_void_p),
        ("k_cache", C.c_void_p),
        ("v_cache", C.c_void_p),
        ("cu_seqlens", C.c_void_p),
        ("cache_seqlens", C.c_void_p),
        ("block_table", C.c_void_p),
        ("rotary_cos", C.c_void_p),
        ("rotary_sin", C.c_void_p),
        ("B", C.c_int32),
        ("total_new", C.c_int32),
        ("Hk", C.c_int32),
        ("D", C.c_int32),
        ("capacity", C.c_int32),
        ("page_size", C.c_int32),
        ("num_pages", C.c_int32),
        ("rotary_dim", C.c_int32),
        ("seqlen_ro", C.c_int32),
        ("rotary_interleaved", C.c_int32),
        ("dtype", C.c_int32),
        ("cs_dtype", C.c_int32),
        ("k_stride", C.c_int64 * 2),
        ("v_stride", C.c_int64 * 2),
        ("kc_stride", C.c_int64 * 3),
        ("vc_stride", C.c_int64 * 3),
        ("block_table_stride", C.c_int64),
        ("cos_stride", C.c_int64),
        ("sin_stride", C.c_int64),
        ("reserved_", C.c_int64),
    ]


class TfaAppendQ(C.Structure):
    """struct tfa_append_q (include/tfa.h): the q that tfa_kvcache_append_varlen_ex rotates in place, handed over beside TfaKvcacheAppendVarlenParams."""

    _fields_ = [
        ("q", C.c_void_p),
        ("H", C.c_int32),
        ("reserved_", C.c_int32),
        ("q_stride", C.c_int64 * 2),
    ]


class TfaError(RuntimeError):
    def __init__(self, status, text):
        super().__init__(f"tfa status {status}: {text}")
        self.status = status


_lib = None


def lib():
    """Load (once) and return the C-ABI library.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C tiny-flash-attention_amd/csrc`. There is no fallback path."
        )
    L = C.CDLL(LIB_PATH)
    P = C.POINTER(TfaFwdParams)
    L.tfa_version.restype = C.c_int
    L.tfa_strerror.restype = C.c_char_p
    L.tfa_strerror.argtypes = [C.c_int]
    L.tfa_fwd.restype = C.c_int
    L.tfa_fwd.argtypes = [P, C.c_void_p]
    bhnd = [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_float, C.c_int, C.c_int, C.c_void_p]
    L.tfa_fwd_bhnd.restype = C.c_int
    L.tfa_fwd_bhnd.argtypes = bhnd
    L.tfa_fwd_bhnd_f32out.restype = C.c_int
    L.tfa_fwd_bhnd_f32out.argtypes = bhnd
    L.tfa_fwd_plan.restype = C.c_int
    L.tfa_fwd_plan.argtypes = [P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.tfa_fwd_time.restype = C.c_int
    L.tfa_fwd_time.argtypes = [P, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_float)]
    L.tfa_set_variant.restype = C.c_int
    L.tfa_set_variant.argtypes = [C.c_int]
    L.tfa_get_variant.restype = C.c_int
    L.tfa_fwd_variant.restype = C.c_int
    L.tfa_fwd_variant.argtypes = [P]
    L.tfa_fwd_rounding_rule.restype = C.c_int
    L.tfa_fwd_rounding_rule.argtypes = [P]
    L.tfa_num_variants.restype = C.c_int
    L.tfa_variant_name.restype = C.c_char_p
    L.tfa_variant_name.argtypes = [C.c_int]
    L.tfa_variant_available.restype = C.c_int
    L.tfa_variant_available.argtypes = [C.c_int]
    L.tfa_debug_set_flags.restype = C.c_int
    L.tfa_debug_set_flags.argtypes = [C.c_int]
    L.tfa_debug_set_trace.restype = C.c_int
    L.tfa_debug_set_trace.argtypes = [C.c_void_p]
    L.tfa_debug_mfma_ceiling.restype = C.c_int
    L.tfa_debug_mfma_ceiling.argtypes = [C.c_void_p, C.c_ulonglong, C.c_double, C.c_void_p, C.POINTER(C.c_double)]
    L.tfa_fwd_splitkv.restype = C.c_int
    L.tfa_fwd_splitkv.argtypes = [P, C.c_int, C.c_void_p, C.c_void_p]
    L.tfa_fwd_suggest_splits.restype = C.c_int
    L.tfa_fwd_suggest_splits.argtypes = [P]
    L.tfa_fwd_splitkv_workspace.restype = C.c_longlong
    L.tfa_fwd_splitkv_workspace.argtypes = [P, C.c_int]
    L.tfa_merge.restype = C.c_int
    L.tfa_merge.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    PB = C.POINTER(TfaBwdParams)
    L.tfa_bwd.restype = C.c_int
    L.tfa_bwd.argtypes = [PB, C.c_void_p]
    L.tfa_bwd_plan.restype = C.c_int
    L.tfa_bwd_plan.argtypes = [PB]
    L.tfa_bwd_work.restype = C.c_int
    L.tfa_bwd_work.argtypes = [PB, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.tfa_bwd_time.restype = C.c_int
    L.tfa_bwd_time.argtypes = [PB, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_float)]
    L.tfa_fwd_work.restype = C.c_int
    L.tfa_fwd_work.argtypes = [P, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    PV = C.POINTER(TfaVarlenFwdParams)
    L.tfa_fwd_varlen.restype = C.c_int
    L.tfa_fwd_varlen.argtypes = [PV, C.c_void_p]
    L.tfa_fwd_varlen_plan.restype = C.c_int
    L.tfa_fwd_varlen_plan.argtypes = [PV, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.tfa_fwd_varlen_variant.restype = C.c_int
    L.tfa_fwd_varlen_variant.argtypes = [PV]
    L.tfa_fwd_varlen_rounding_rule.restype = C.c_int
    L.tfa_fwd_varlen_rounding_rule.argtypes = [PV]
    L.tfa_bwd_varlen.restype = C.c_int
    L.tfa_bwd_varlen.argtypes = [C.POINTER(TfaVarlenBwdParams), C.c_void_p]
    PG = C.POINTER(TfaPagedKv)
    for name, args in (("tfa_fwd_varlen_paged", [PV, PG, C.c_void_p]),
                       ("tfa_fwd_varlen_paged_plan", [PV, PG, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
                       ("tfa_fwd_varlen_paged_variant", [PV, PG]), ("tfa_fwd_varlen_paged_rounding_rule", [PV, PG])):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = args
    IP = C.POINTER(C.c_int)
    PF = C.POINTER(TfaFwdParams)
    PB = C.POINTER(TfaBwdParams)
    PVB = C.POINTER(TfaVarlenBwdParams)
    for name, args in (("tfa_fwd_local", [PF, C.c_int, C.c_int, C.c_void_p]), ("tfa_fwd_local_plan", [PF, C.c_int, C.c_int, IP, IP, IP]),
                       ("tfa_fwd_local_variant", [PF, C.c_int, C.c_int]), ("tfa_fwd_local_rounding_rule", [PF, C.c_int, C.c_int]),
                       ("tfa_fwd_varlen_local", [PV, C.c_int, C.c_int, C.c_void_p]), ("tfa_fwd_varlen_local_plan", [PV, C.c_int, C.c_int, IP, IP, IP]),
                       ("tfa_fwd_varlen_local_variant", [PV, C.c_int, C.c_int]), ("tfa_fwd_varlen_local_rounding_rule", [PV, C.c_int, C.c_int]),
                       ("tfa_bwd_local", [PB, C.c_int, C.c_int, C.c_void_p]), ("tfa_bwd_local_plan", [PB, C.c_int, C.c_int]),
                       ("tfa_bwd_varlen_local", [PVB, C.c_int, C.c_int, C.c_void_p]), ("tfa_bwd_varlen_local_plan", [PVB, C.c_int, C.c_int])):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = args
    # ALiBi: the local entry points' arguments with (const float* alibi_slopes, int64_t slopes_batch_stride) in front of the window
    AL = [C.c_void_p, C.c_int64, C.c_int, C.c_int]
    for name, args in (("tfa_fwd_alibi", [PF] + AL + [C.c_void_p]), ("tfa_fwd_alibi_plan", [PF] + AL + [IP, IP, IP]),
                       ("tfa_fwd_alibi_variant", [PF] + AL), ("tfa_fwd_alibi_rounding_rule", [PF] + AL),
                       ("tfa_fwd_varlen_alibi", [PV] + AL + [C.c_void_p]), ("tfa_fwd_varlen_alibi_plan", [PV] + AL + [IP, IP, IP]),
                       ("tfa_fwd_varlen_alibi_variant", [PV] + AL), ("tfa_fwd_varlen_alibi_rounding_rule", [PV] + AL),
                       ("tfa_bwd_alibi", [PB] + AL + [C.c_void_p]), ("tfa_bwd_alibi_plan", [PB] + AL),
                       ("tfa_bwd_varlen_alibi", [PVB] + AL + [C.c_void_p]), ("tfa_bwd_varlen_alibi_plan", [PVB] + AL)):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = args
    # soft-capping: the ALiBi entry points' arguments with (float softcap) in front of the slopes, which may be NULL
    SC = [C.c_float] + AL
    for name, args in (("tfa_fwd_softcap", [PF] + SC + [C.c_void_p]), ("tfa_fwd_softcap_plan", [PF] + SC + [IP, IP, IP]),
                       ("tfa_fwd_softcap_variant", [PF] + SC), ("tfa_fwd_softcap_rounding_rule", [PF] + SC),
                       ("tfa_fwd_varlen_softcap", [PV] + SC + [C.c_void_p]), ("tfa_fwd_varlen_softcap_plan", [PV] + SC + [IP, IP, IP]),
                       ("tfa_fwd_varlen_softcap_variant", [PV] + SC), ("tfa_fwd_varlen_softcap_rounding_rule", [PV] + SC),
                       ("tfa_bwd_softcap", [PB] + SC + [C.c_void_p]), ("tfa_bwd_softcap_plan", [PB] + SC),
                       ("tfa_bwd_varlen_softcap", [PVB] + SC + [C.c_void_p]), ("tfa_bwd_varlen_softcap_plan", [PVB] + SC)):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = args
    # dense bias: the local entry points' arguments with (const tfa_attn_bias* bias) in front of the window
    BI = [C.POINTER(TfaAttnBias), C.c_int, C.c_int]
    for name, args in (("tfa_fwd_bias", [PF] + BI + [C.c_void_p]), ("tfa_fwd_bias_plan", [PF] + BI + [IP, IP, IP]),
                       ("tfa_fwd_bias_variant", [PF] + BI), ("tfa_fwd_bias_rounding_rule", [PF] + BI),
                       ("tfa_bwd_bias", [PB] + BI + [C.c_void_p]), ("tfa_bwd_bias_plan", [PB] + BI)):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = args
    # attention over a K/V cache (tfa_kvcache_params)
    PK = C.POINTER(TfaKvcacheParams)
    L.tfa_fwd_kvcache.restype = C.c_int
    L.tfa_fwd_kvcache.argtypes = [PK, C.c_int, C.c_void_p, C.c_void_p]
    L.tfa_fwd_kvcache_workspace.restype = C.c_longlong
    L.tfa_fwd_kvcache_workspace.argtypes = [PK, C.c_int]
    L.tfa_fwd_kvcache_plan.restype = C.c_int
    L.tfa_fwd_kvcache_plan.argtypes = [PK, C.c_int, IP, IP, IP]
    L.tfa_fwd_kvcache_suggest_splits.restype = C.c_int
    L.tfa_fwd_kvcache_suggest_splits.argtypes = [PK]
    L.tfa_kvcache_append.restype = C.c_int
    L.tfa_kvcache_append.argtypes = [PK, C.c_void_p]
    # ... with an e4m3 cache (tfa_kvcache_fp8)
    P8 = C.POINTER(TfaKvcacheFp8)
    L.tfa_fwd_kvcache_fp8.restype = C.c_int
    L.tfa_fwd_kvcache_fp8.argtypes = [PK, P8, C.c_int, C.c_void_p, C.c_void_p]
    L.tfa_fwd_kvcache_fp8_workspace.restype = C.c_longlong
    L.tfa_fwd_kvcache_fp8_workspace.argtypes = [PK, P8, C.c_int]
    L.tfa_fwd_kvcache_fp8_plan.restype = C.c_int
    L.tfa_fwd_kvcache_fp8_plan.argtypes = [PK, P8, C.c_int, IP, IP, IP]
    L.tfa_kvcache_append_fp8.restype = C.c_int
    L.tfa_kvcache_append_fp8.argtypes = [PK, P8, C.c_void_p]
    # ... with the GQA packing chosen by the caller (TFA_PACK_GQA_*; P8 may be None: the 16-bit cache)
    L.tfa_fwd_kvcache_pack.restype = C.c_int
    L.tfa_fwd_kvcache_pack.argtypes = [PK, P8, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.tfa_fwd_kvcache_pack_workspace.restype = C.c_longlong
    L.tfa_fwd_kvcache_pack_workspace.argtypes = [PK, P8, C.c_int, C.c_int]
    L.tfa_fwd_kvcache_pack_plan.restype = C.c_int
    L.tfa_fwd_kvcache_pack_plan.argtypes = [PK, P8, C.c_int, C.c_int, IP, IP, IP]
    L.tfa_fwd_kvcache_pack_suggest_splits.restype = C.c_int
    L.tfa_fwd_kvcache_pack_suggest_splits.argtypes = [PK, C.c_int]
    # ... for packed ragged query rows (tfa_kvcache_varlen_q: cu_seqlens_q on the device)
    PV = C.POINTER(TfaKvcacheVarlenQ)
    L.tfa_fwd_kvcache_varlen.restype = C.c_int
    L.tfa_fwd_kvcache_varlen.argtypes = [PK, PV, P8, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.tfa_fwd_kvcache_varlen_workspace.restype = C.c_longlong
    L.tfa_fwd_kvcache_varlen_workspace.argtypes = [PK, PV, P8, C.c_int, C.c_int]
    L.tfa_fwd_kvcache_varlen_plan.restype = C.c_int
    L.tfa_fwd_kvcache_varlen_plan.argtypes = [PK, PV, P8, C.c_int, C.c_int, IP, IP, IP]
    L.tfa_fwd_kvcache_varlen_suggest_splits.restype = C.c_int
    L.tfa_fwd_kvcache_varlen_suggest_splits.argtypes = [PK, PV, C.c_int]
    # ... and its scheduled form: the work list built on the device (metadata: int32 in device memory), then the attention call that runs from it
    L.tfa_kvcache_varlen_schedule_size.restype = C.c_longlong
    L.tfa_kvcache_varlen_schedule_size.argtypes = [PK, PV, C.c_int, C.c_int]
    L.tfa_kvcache_varlen_schedule.restype = C.c_int
    L.tfa_kvcache_varlen_schedule.argtypes = [PK, PV, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.tfa_kvcache_varlen_schedule_plan.restype = C.c_int
    L.tfa_kvcache_varlen_schedule_plan.argtypes = [PK, PV, C.c_int, C.c_int, IP, IP, IP]
    L.tfa_fwd_kvcache_varlen_sched.restype = C.c_int
    L.tfa_fwd_kvcache_varlen_sched.argtypes = [PK, PV, P8, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tfa_fwd_kvcache_varlen_sched_plan.restype = C.c_int
    L.tfa_fwd_kvcache_varlen_sched_plan.argtypes = [PK, PV, P8, C.c_int, C.c_int, IP, IP, IP]
    # ... and a sliding window over the cache, one entry point for every form (PV None: the 4-D call; the metadata pointer None: unscheduled)
    L.tfa_fwd_kvcache_window.restype = C.c_int
    L.tfa_fwd_kvcache_window.argtypes = [PK, PV, P8, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tfa_fwd_kvcache_window_plan.restype = C.c_int
    L.tfa_fwd_kvcache_window_plan.argtypes = [PK, PV, P8, C.c_int, C.c_int, C.c_int, C.c_int, IP, IP, IP]
    L.tfa_fwd_kvcache_window_workspace.restype = C.c_longlong
    L.tfa_fwd_kvcache_window_workspace.argtypes = [PK, PV, P8, C.c_int, C.c_int, C.c_int]
    L.tfa_fwd_kvcache_window_suggest_splits.restype = C.c_int
    L.tfa_fwd_kvcache_window_suggest_splits.argtypes = [PK, PV, C.c_int, C.c_int]
    # ... and a speculative tree's visibility words over the step's new keys, the same shape of entry point (the window's integer replaced by the tfa_kvcache_tree)
    PT = C.POINTER(TfaKvcacheTree)
    L.tfa_fwd_kvcache_tree.restype = C.c_int
    L.tfa_fwd_kvcache_tree.argtypes = [PK, PV, P8, C.c_int, PT, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tfa_fwd_kvcache_tree_plan.restype = C.c_int
    L.tfa_fwd_kvcache_tree_plan.argtypes = [PK, PV, P8, C.c_int, PT, C.c_int, C.c_int, IP, IP, IP]
    L.tfa_fwd_kvcache_tree_workspace.restype = C.c_longlong
    L.tfa_fwd_kvcache_tree_workspace.argtypes = [PK, PV, P8, C.c_int, PT, C.c_int]
    L.tfa_fwd_kvcache_tree_suggest_splits.restype = C.c_int
    L.tfa_fwd_kvcache_tree_suggest_splits.argtypes = [PK, PV, C.c_int, PT]
    # ... and shared-prefix (cascade) attention: the packed-q call over each sequence's own keys plus the tfa_kvcache_cascade of the groups' shared keys
    PC = C.POINTER(TfaKvcacheCascade)
    L.tfa_fwd_kvcache_cascade.restype = C.c_int
    L.tfa_fwd_kvcache_cascade.argtypes = [PK, PV, PC, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tfa_fwd_kvcache_cascade_workspace.restype = C.c_longlong
    L.tfa_fwd_kvcache_cascade_workspace.argtypes = [PK, PV, PC, C.c_int, C.c_int, C.c_int]
    L.tfa_fwd_kvcache_cascade_plan.restype = C.c_int
    L.tfa_fwd_kvcache_cascade_plan.argtypes = [PK, PV, PC, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, IP, IP, IP]
    L.tfa_fwd_kvcache_cascade_suggest_splits.restype = C.c_int
    L.tfa_fwd_kvcache_cascade_suggest_splits.argtypes = [PK, PV, PC, C.c_int, IP, IP]
    # rotary embedding (tfa_rotary_params) and the packed append (tfa_kvcache_append_varlen_params)
    PR, PA = C.POINTER(TfaRotaryParams), C.POINTER(TfaKvcacheAppendVarlenParams)
    for name, args in (("tfa_rotary", [PR, C.c_void_p]), ("tfa_rotary_plan", [PR, IP, IP]),
                       ("tfa_kvcache_append_varlen", [PA, C.c_void_p]), ("tfa_kvcache_append_varlen_plan", [PA, IP, IP]),
                       # ... into an e4m3 cache and / or with q rotated in the launch (P8 / the tfa_append_q may be None)
                       ("tfa_kvcache_append_varlen_ex", [PA, P8, C.POINTER(TfaAppendQ), C.c_void_p]),
                       ("tfa_kvcache_append_varlen_ex_plan", [PA, P8, C.POINTER(TfaAppendQ), IP, IP])):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = args
    _lib = L
    return L


def check(status):
    if status != 0:
        raise TfaError(status, lib().tfa_strerror(status).decode())


def strerror(status):
    return lib().tfa_strerror(status).decode()


def set_variant(v):
    check(lib().tfa_set_variant(int(v)))


def debug_set_flags(flags):
    """Bring-up flags of the calling thread (include/tfa.h: tfa_debug_set_flags); 0 = normal."""
    check(lib().tfa_debug_set_flags(int(flags)))


def debug_bwd_split(on):
    """tfa_debug_bwd_split: dK and dV as two launches (A/B and cross-check of the fused dK/dV kernel)."""
    check(lib().tfa_debug_bwd_split(int(on)))       # bit 0: two-launch dK/dV form; bit 1: force the windowed (>= 2 GiB) instantiations


def get_variant():
    return lib().tfa_get_variant()


def num_variants():
    return lib().tfa_num_variants()


def variant_available(v):
    """True when kernel variant `v` is compiled into the loaded library (the product build carries only the
    dispatched kernels; A/B arms need `make EXPERIMENTAL=1`)."""
    return bool(lib().tfa_variant_available(int(v)))


def variant_name(v):
    return lib().tfa_variant_name(int(v)).decode()


def variant_for(B, H, Hk, Nq, Nk, D, is_causal, dtype=TFA_BF16, flags=0):
    """The variant tfa_fwd would run for a contiguous (B,H,N,D) problem of these sizes (no GPU needed)."""
    p = TfaFwdParams()
    p.q = p.k = p.v = p.out = 0x1000           # never dereferenced: tfa_fwd_variant only validates and plans
    p.lse = None
    p.B, p.H, p.Hk, p.Nq, p.Nk, p.D = B, H, Hk, Nq, Nk, D
    for name, n, h in (("q_stride", Nq, H), ("k_stride", Nk, Hk), ("v_stride", Nk, Hk), ("o_stride", Nq, H)):
        arr = getattr(p, name)
        arr[0], arr[1], arr[2] = h * n * D, n * D, D
    p.softmax_scale = 1.0
    p.is_causal = 1 if is_causal else 0
    p.dtype = p.out_dtype = dtype
    p.flags = flags
    v = lib().tfa_fwd_variant(C.byref(p))
    if v < 0:
        check(v)
    return v


RULE_EXACT_MAX, RULE_LAZY, RULE_FIRST_TILE = 0, 1, 2


def rounding_rule(p):
    """The row reference tfa_fwd rounds P against for the problem *p (include/tfa.h: TFA_RULE_*)."""
    r = lib().tfa_fwd_rounding_rule(C.byref(p))
    if r < 0:
        check(r)
    return r


def rule_for(B, H, Hk, Nq, Nk, D, is_causal, dtype=TFA_BF16, flags=0):
    """rounding_rule for a contiguous (B,H,N,D) problem of these sizes (no GPU needed); honours a forced variant like variant_for."""
    p = TfaFwdParams()
    p.q = p.k = p.v = p.out = 0x1000
    p.lse = None
    p.B, p.H, p.Hk, p.Nq, p.Nk, p.D = B, H, Hk, Nq, Nk, D
    for name, n, h in (("q_stride", Nq, H), ("k_stride", Nk, Hk), ("v_stride", Nk, Hk), ("o_stride", Nq, H)):
        arr = getattr(p, name)
        arr[0], arr[1], arr[2] = h * n * D, n * D, D
    p.softmax_scale = 1.0
    p.is_causal = 1 if is_causal else 0
    p.dtype = p.out_dtype = dtype
    p.flags = flags
    return rounding_rule(p)


def lazy_reference(v):
    """True for the variants that keep a lazily re-based row reference instead of the exact running max (names "il..." / "x4...";
    "exact-il8", variant 38, is the il8 kernel with the exact running max)."""
    return variant_name(v).startswith("il") or variant_name(v).startswith("x4")
