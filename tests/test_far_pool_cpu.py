"""tests/far_pool.py's placement proved on the CPU, for every case tests/test_far_pool_gpu.py runs: every case of kvcache_ref, kvcache_window_ref and
kvcache_tree_ref, fwd_ref's paged cases, far_pool.EXTRA and the plain-launch appends, and 16 seeded draws of each module.  No arena: the pool is modelled sparsely
(far_pool.Sparse: the placed slots' bytes, 0xFF — NaN in every cache type — everywhere else).

    logical keys   gathering through the far table returns the keys kvcache_ref.gather returns from the small pool, bit for bit: the fp64 references are reused
    geometry       every placed byte inside the arena, bases and batch strides 16-byte aligned, every index in [0, num_pages), no index twice
    alias rule     none of the eight truncation mutants of any placed slot lands inside any placed slot
    mutants        every mutant that changes the address of a key a live row reads makes the sparse gather of that row's keys contain a NaN; a mutant that
                   changes none carries a structural reason; a case may leave out all eight only as a contiguous cache of one sequence (the far offset is then in
                   the base pointer: far_pool.B1_REASON); over each family every one of the eight applies to at least one case — for an append launch, to rows
                   the append stores
    the bounds     a K read through a truncated page base fails the family's out and lse bounds (what a kernel with `(int)(page * ks_b)` would show)
    plans          the host plans the far geometry as it plans the small one: TFA_OK, the same grid, block, LDS bytes, variant and split count — which is what
                   entitles the GPU test to demand identical bits
"""
import ctypes as C
import functools

import pytest
import torch

import far_pool as FP
import kvcache_ref as K
import kvcache_tree_ref as T
import kvcache_window_ref as W
from tiny_flash_attention_amd import _lib

MODS = FP.modules()
IDS = [(name, cid) for name, (_, ids) in MODS.items() for cid in ids] + [("append_varlen", f"{kind}:{page}") for kind in FP.APPEND_VARLEN for page in (64, 0)]
ADDR = 0x10000          # a 16-byte aligned stand-in for device pointers (plans never dereference them)
case_param = pytest.mark.parametrize("name,cid", IDS, ids=[f"{n}/{c}" for n, c in IDS])


@functools.lru_cache(maxsize=None)
def placed(name, cid):
    if name == "append_varlen":
        kind, page = cid.split(":")
        t = FP.append_varlen_case(kind, page=int(page))
    else:
        mod = MODS[name][0]
        t = mod.build(FP.case_of(mod, cid))
    return t, FP.place(t)


def nan_equal(a, b):
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


@case_param
def test_far_table_gathers_the_small_pools_keys(name, cid):
    t, pl = placed(name, cid)
    L = pl.L
    sp = FP.Sparse(pl)
    n = L["bt"].shape[1] * L["rows"] if pl.paged else L["rows"]
    for b in range(L["B"]):
        for which, cache in (("k", L["kc"]), ("v", L["vc"])):
            assert nan_equal(sp.gather(which, b, 0, n).float().double(), K.gather(cache, L["bt"], b, n)), f"{cid}: {which} of sequence {b}"


@case_param
def test_geometry(name, cid):
    t, pl = placed(name, cid)
    L = pl.L
    starts = [pl.start(i) for i in range(len(pl.far))]
    assert all(0 <= s and s + pl.slot_bytes <= FP.ARENA_BYTES for s in starts), "a placed byte outside the arena"
    assert all(s % 16 == 0 for s in starts) and pl.ptr_v % 16 == 0 and (pl.stride * pl.es) % 16 == 0
    assert len(set(starts)) == len(starts) and all(b - a >= pl.slot_bytes for a, b in zip(sorted(starts), sorted(starts)[1:])), "two slots overlap"
    if pl.paged:
        assert pl.num_pages == FP.ARENA_BYTES // pl.slot_bytes and pl.stride == 2 * L["rows"] * L["Hk"] * L["D"]
        assert all(0 <= f < pl.num_pages for f in pl.far) and len(pl.far) == L["kc"].shape[0]
        assert pl.bt.dtype == torch.int32 and pl.bt.shape == L["bt"].shape and int(pl.bt.min()) >= 0 and int(pl.bt.max()) < pl.num_pages
        assert pl.num_pages >= 2 ** 14 + 128               # (the largest page among the cases: 256 KiB, twice in the interleaved layout)
    elif L["B"] > 1:
        assert pl.ptr_k == 0 and 2 ** 31 <= pl.stride * pl.es and pl.start(L["B"] - 1) >= 2 ** 33 - 2 ** 20
    else:
        assert pl.ptr_k + pl.slot_bytes > FP.ARENA_BYTES - 16


@case_param
def test_alias_rule(name, cid):
    t, pl = placed(name, cid)
    assert pl.alias_free(), f"{cid}: a truncated offset of a placed slot lands inside a placed slot"


@case_param
def test_every_mutant_that_applies_bites_and_the_others_say_why(name, cid):
    t, pl = placed(name, cid)
    L = pl.L
    ok, na = pl.mutants()
    assert len(ok) + len(na) == 8 and all(why for _, why in na)
    if len(na) == 8:
        assert not pl.paged and L["B"] == 1 and {why for _, why in na} == {FP.B1_REASON}, f"{cid} leaves out all eight mutants"
    if pl.paged or L["B"] > 1:
        assert ok, f"{cid}: no mutant applies"
    sp = FP.Sparse(pl)
    for m in ok:
        b, lo, hi = next(r for r in L["live"] if pl.changed(m, [r]))
        got = sp.gather("k", b, lo, hi, m).float()
        true = sp.gather("k", b, lo, hi).float()
        assert bool(torch.isnan(got).any()), f"{cid}: {FP.mname(m)} changes an address of sequence {b} and reads no NaN"
        assert bool(torch.isnan(sp.gather("v", b, lo, hi, m).float()).any())
        same = (got == true).all(dim=-1).all(dim=-1)       # the keys whose address the mutant leaves alone read as they are
        assert bool((same | torch.isnan(got).any(dim=-1).any(dim=-1)).all()), f"{cid}: {FP.mname(m)} reads a foreign key, not NaN"


def test_every_mutant_applies_in_every_family():
    seen = {f: set() for f in FP.FAMILIES}
    for name, cid in IDS:
        t, pl = placed(name, cid)
        for fam in FP.families(name, t["case"]):
            ranges = pl.L["written"] if fam.startswith("launch") else None
            seen[fam] |= set(pl.mutants(ranges)[0])
    for fam, ms in seen.items():
        assert ms == set(FP.MUTANTS), f"{fam}: no case where {sorted(FP.mname(m) for m in set(FP.MUTANTS) - ms)} apply"


def test_thresholds_crossed_in_every_family():
    """Every family has a case whose live keys (an append launch: the rows it stores) sit beyond 2^31, 2^32 and 2^33 bytes."""
    seen = {f: set() for f in FP.FAMILIES}
    for name, cid in IDS:
        t, pl = placed(name, cid)
        for fam in FP.families(name, t["case"]):
            ranges = pl.L["written"] if fam.startswith("launch") else pl.L["live"]
            seen[fam] |= {th for th, v in pl.beyond(ranges).items() if v}
    for fam, ths in seen.items():
        assert ths == set(FP.THRESHOLDS), f"{fam}: thresholds crossed {sorted(ths)}"


# ---- a truncated read fails the bounds -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cid", [("kvcache", "4d-fp16-d64-g2-nq5-causal-page64-s2"), ("kvcache", "4d-fp8-bf16-d112-g1-nq1-page64-s2"), ("kvcache", "4d-bf16-d40-g1-nq1"),
                                      ("window", "w4d-bf16-d104-g4-nq1-w64-page128-s3"), ("tree", "t4d-bf16-d104-g4-nq33-page128-s3-pack")])
def test_a_truncated_page_base_fails_the_bounds(name, cid):
    """K read as a kernel whose page (or batch) base product is an int would read it — (int)(page * ks_b): the mutant s32-elements-page — put through the family's
    definition: out and lse leave their bounds (a NaN counts as infinitely far out)."""
    t, pl = placed(name, cid)
    c = t["case"]
    m = ("s32", "elements", "page")
    problem = {"kvcache": K.seq_problem, "window": W.win_problem, "tree": T.tree_problem}[name]
    ref = MODS[name][0].reference(t)
    sp = FP.Sparse(pl, final=True)
    b, lo, hi = next(r for r in pl.L["live"] if pl.changed(m, [r]))
    p = problem(t, b)
    hk_of = torch.arange(c["H"]) // (c["H"] // c["Hk"])
    assert nan_equal(sp.gather("k", b, 0, hi).float().double()[:, hk_of].transpose(0, 1), p["k"]), "the sparse model is the definition's K"
    p["k"] = sp.gather("k", b, 0, hi, m).float().double()[:, hk_of].transpose(0, 1)
    out, lse, _, _ = K.attend(p)
    r_out, r_lse, A, Tm, n = ref[b]
    assert K.out_ratio(out, r_out, A, t["dtype"]) > 1.0 and K.lse_ratio(lse, r_lse, Tm, n, c["D"], K.lse_splits(c)) > 1.0


# ---- the host plans the far geometry as the small one ----------------------------------------------------------------------------------------------------------
def ref(x):
    return C.byref(x) if x is not None else None


def tfa_dtype(dt):
    return _lib.TFA_BF16 if dt == torch.bfloat16 else _lib.TFA_F16


def cache_fields(p, names, L, pl, t):
    """The cache pointers, strides and table fields of a params struct for the small pool (pl None) or the far placement."""
    rows, hd, D = L["rows"], L["Hk"] * L["D"], L["D"]
    if pl is None:
        kb, ptr_v, num_pages = rows * hd, (L["kc"].numel() * L["es"] + 15) // 16 * 16, L["kc"].shape[0]
        ptr_k = 0
    else:
        kb, ptr_k, ptr_v, num_pages = pl.stride, pl.ptr_k, pl.ptr_v, pl.num_pages
    p.k_cache, p.v_cache = ADDR + ptr_k, ADDR + ptr_v
    for nm in names:
        arr = getattr(p, nm)
        arr[0], arr[1], arr[2] = kb, D, hd
    if L["bt"] is not None:
        p.block_table, p.block_table_stride, p.page_size, p.num_pages = ADDR, L["bt"].shape[1], rows, num_pages


def fp8_struct(Hk):
    s = _lib.TfaKvcacheFp8()
    s.format, s.k_descale, s.v_descale = _lib.TFA_KV_E4M3, ADDR, ADDR
    for arr in (s.k_descale_stride, s.v_descale_stride):
        arr[0], arr[1] = Hk, 1
    return s


def kvcache_plan(name, t, pl):
    """(status, grid, block, lds, splits) of the attention call of a kvcache / window / tree case over the small pool (pl None) or the far one."""
    lib = _lib.lib()
    c, L = t["case"], FP.layout(t)
    H, Hk, D = c["H"], c["Hk"], c["D"]
    p = _lib.TfaKvcacheParams()
    p.q = p.out = p.lse = p.cache_seqlens = ADDR
    p.B, p.H, p.Hk, p.D, p.capacity = t["B"], H, Hk, D, c["cap"]
    vq = None
    if c["form"] == "4d":
        Nq = c["Nq"]
        p.Nq = Nq
        p.q_stride[0], p.q_stride[1], p.q_stride[2] = Nq * H * D, D, H * D
        p.o_stride[0], p.o_stride[1], p.o_stride[2] = H * Nq * D, Nq * D, D
    else:
        p.q_stride[0], p.q_stride[1], p.q_stride[2] = 0, D, H * D
        p.o_stride[0], p.o_stride[1], p.o_stride[2] = 0, t["total_q"] * D, D
        vq = _lib.TfaKvcacheVarlenQ()
        vq.cu_seqlens_q, vq.max_seqlen_q, vq.total_q = ADDR, c["max_q"], t["total_q"]
    cache_fields(p, ("k_stride", "v_stride"), L, pl, t)
    if c["append"] == "4d":
        p.k_new = p.v_new = ADDR
        p.n_new = c["n_new"]
        for nm in ("knew_stride", "vnew_stride"):
            arr = getattr(p, nm)
            arr[0], arr[1], arr[2] = c["n_new"] * Hk * D, D, Hk * D
    p.softmax_scale, p.is_causal, p.dtype = t["sc"], int(c["causal"]), tfa_dtype(t["dtype"])
    q8 = fp8_struct(Hk) if c["fp8"] else None
    mode = {None: 0, True: 1, False: 2}[c["pack"]]
    sched = int(bool(c["sched"]))
    g, b, l = C.c_int(), C.c_int(), C.c_int()
    out = (C.byref(g), C.byref(b), C.byref(l))
    if name == "window":
        left = c["w"] - 1
        splits = c["splits"] or lib.tfa_fwd_kvcache_window_suggest_splits(ref(p), ref(vq), mode, left)
        st = lib.tfa_fwd_kvcache_window_plan(ref(p), ref(vq), ref(q8), mode, left, splits, sched, *out)
    elif name == "tree":
        tr = _lib.TfaKvcacheTree()
        tr.mask, tr.batch_stride, tr.row_stride = ADDR, (c["Nq"] if c["form"] == "4d" else 0), 1
        splits = c["splits"] or lib.tfa_fwd_kvcache_tree_suggest_splits(ref(p), ref(vq), mode, ref(tr))
        st = lib.tfa_fwd_kvcache_tree_plan(ref(p), ref(vq), ref(q8), mode, ref(tr), splits, sched, *out)
    elif vq is not None:
        splits = c["splits"] or lib.tfa_fwd_kvcache_varlen_suggest_splits(ref(p), ref(vq), mode)
        fn = lib.tfa_fwd_kvcache_varlen_sched_plan if sched else lib.tfa_fwd_kvcache_varlen_plan
        st = fn(ref(p), ref(vq), ref(q8), mode, splits, *out)
    else:
        splits = c["splits"] or lib.tfa_fwd_kvcache_pack_suggest_splits(ref(p), mode)
        st = lib.tfa_fwd_kvcache_pack_plan(ref(p), ref(q8), mode, splits, *out)
    return st, g.value, b.value, l.value, splits


def append_plan(t, pl):
    """(status, grid, block) of the packed append of a case: tfa_kvcache_append_varlen_plan for the plain launch, _ex_plan with q= / fp8."""
    lib = _lib.lib()
    c, L = t["case"], FP.layout(t)
    Hk, D = c["Hk"], c["D"]
    p = _lib.TfaKvcacheAppendVarlenParams()
    p.k, p.v, p.cu_seqlens, p.cache_seqlens = ADDR, 2 * ADDR, 5 * ADDR, 6 * ADDR
    p.B, p.total_new, p.Hk, p.D, p.capacity = t["B"], t["k_new"].shape[0], Hk, D, c["cap"]
    for nm in ("k_stride", "v_stride"):
        arr = getattr(p, nm)
        arr[0], arr[1] = D, Hk * D
    cache_fields(p, ("kc_stride", "vc_stride"), L, pl, t)
    if t["cos"] is not None:
        p.rotary_cos, p.rotary_sin = 8 * ADDR, 9 * ADDR
        p.rotary_dim, p.seqlen_ro, p.cos_stride, p.sin_stride = D, t["cos"].shape[0], D // 2, D // 2
        p.rotary_interleaved = int(c.get("kind") == "interleaved")
        p.cs_dtype = tfa_dtype(t["dtype"])
    p.dtype = tfa_dtype(t["dtype"])
    g, b = C.c_int(), C.c_int()
    if c["append"] == "plain":
        return lib.tfa_kvcache_append_varlen_plan(ref(p), C.byref(g), C.byref(b)), g.value, b.value
    rq = _lib.TfaAppendQ()
    rq.q, rq.H = 12 * ADDR, c["H"]
    rq.q_stride[0], rq.q_stride[1] = D, c["H"] * D
    return lib.tfa_kvcache_append_varlen_ex_plan(ref(p), ref(fp8_struct(Hk) if c["fp8"] else None), ref(rq), C.byref(g), C.byref(b)), g.value, b.value


def prefill_plan(t, pl):
    """(status, grid, block, lds, variant) of tfa_fwd_varlen_paged for a paged case of fwd_ref."""
    lib = _lib.lib()
    c, L = t["case"], FP.layout(t)
    H, Hk, D = c["H"], c["Hk"], c["D"]
    p = _lib.TfaVarlenFwdParams()
    p.q = p.out = p.lse = p.cu_seqlens_q = p.cu_seqlens_k = ADDR
    p.k, p.v = (ADDR, ADDR + (L["kc"].numel() * 2 + 15) // 16 * 16) if pl is None else (ADDR + pl.ptr_k, ADDR + pl.ptr_v)
    p.B, p.H, p.Hk, p.D = len(c["lq"]), H, Hk, D
    p.max_seqlen_q, p.max_seqlen_k, p.total_q, p.total_k = max(1, max(c["lq"])), max(1, max(c["lk"])), t["q"].shape[0], 0
    p.q_stride[0], p.q_stride[1] = D, H * D
    p.o_stride[0], p.o_stride[1] = D, H * D
    for nm in ("k_stride", "v_stride"):
        getattr(p, nm)[0], getattr(p, nm)[1] = D, Hk * D
    p.softmax_scale, p.is_causal = t["sc"], int(c["causal"])
    p.dtype = p.out_dtype = tfa_dtype(t["dtype"])
    pg = _lib.TfaPagedKv()
    pg.block_table, pg.table_stride, pg.max_blocks = ADDR, L["bt"].shape[1], L["bt"].shape[1]
    pg.page_size, pg.num_pages = L["rows"], L["kc"].shape[0] if pl is None else pl.num_pages
    pg.k_page_stride = pg.v_page_stride = L["rows"] * Hk * D if pl is None else pl.stride
    g, b, l = C.c_int(), C.c_int(), C.c_int()
    _lib.set_variant(c["variant"])
    try:
        st = lib.tfa_fwd_varlen_paged_plan(ref(p), ref(pg), C.byref(g), C.byref(b), C.byref(l))
        var = lib.tfa_fwd_varlen_paged_variant(ref(p), ref(pg))
    finally:
        _lib.set_variant(-1)
    return st, g.value, b.value, l.value, var


@case_param
def test_the_host_plans_the_far_geometry_as_the_small_one(name, cid):
    t, pl = placed(name, cid)
    c = t["case"]
    plans = []
    if name == "prefill":
        plans.append(prefill_plan)
    elif name == "append_varlen":
        plans.append(append_plan)
    else:
        plans.append(functools.partial(kvcache_plan, name))
        if c["append"] == "varlen":
            plans.append(append_plan)
    for plan in plans:
        small, far = plan(t, None), plan(t, pl)
        assert small[0] == 0, f"{cid}: the small pool's plan is refused ({small})"
        assert far == small, f"{cid}: far plan {far}, small plan {small}"
        assert small[1] >= 1 and small[2] >= 64
