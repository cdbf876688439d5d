"""The fp64 definition of flash_attn_with_kvcache(sliding_window=w), its per-element bounds, the cases tests/test_kvcache_window_gpu.py runs on the GPU and
tests/test_kvcache_window_bounds_cpu.py proves on the CPU, and the window mutants the bounds must tell from the definition (tests only).

The definition is tests/kvcache_ref.py's — seq_problem / attend, unchanged — with `vis` AND-ed with the window (include/tfa.h, tfa_fwd_kvcache_window): with
left = w - 1 and shift_b = len_b - nq_b, key j is visible to row t of sequence b iff  t + shift_b - left <= j <= t + shift_b  and  0 <= j < len_b.  Every case
is causal.  The chunks of num_splits are cut from [lo64_b, len_b), lo_b = max(0, shift_b - left), lo64_b = lo_b & ~63 (win_chunks); the emulations use them.

Bounds: kvcache_ref's, element by element.  out: eps16 * A + 1e-6 + half an ulp16 (A summed over the window's keys).  lse: kvcache_ref.lse_bound with the
tile count of [lo64_b, len_b) — the tiles a chunked loop over the windowed range can visit; a tile in front of a block's first is fully masked for every row of
the block and changes neither m, l nor O, so the emulations below, which walk every tile of a windowed chunk, compute what a loop that starts at each block's
first tile computes.

Inputs: kvcache_ref.build's, plus the weight its hot keys have on the window-edge keys, which build cannot know: for the first and the last row of every
sequence the key just outside the window and the first key inside it, and the last key of every windowed chunk that has a chunk behind it (build()).
"""
import math
import random

import torch

import kvcache_ref as K

WINDOWS = (1, 2, 64, 65, 100, 128, 512)
WMUTANTS = ("left+1", "left-1", "edge_tile_unmasked", "edge_tile_skipped", "first_row_bound", "win_pack_pos", "win_nq_unclamped", "win_seam")


def lo64_of(n, nq, left):
    lo = max(0, n - nq - left)
    return lo & ~63


def win_chunks(n, nq, left, splits):
    """include/tfa.h: chunk_b = round_up(ceil((len_b - lo64_b) / splits), 64), chunk s = [lo64_b + s * chunk_b, min(len_b, lo64_b + (s + 1) * chunk_b))."""
    lo = lo64_of(n, nq, left)
    if splits <= 1:
        return [(lo, n)]
    ch = K.chunk_of(n - lo, splits)
    return [(min(n, lo + s * ch), min(n, lo + (s + 1) * ch)) for s in range(splits)]


def left_bounds(t, b, p, mut=None):
    """(H, nq) the first key each row sees (may be negative), by the definition or by a wrong one (WMUTANTS)."""
    c = t["case"]
    H, nq, n = p["q"].shape[0], p["nq"], p["n"]
    G = c["H"] // c["Hk"]
    left = c["w"] - 1 + {"left+1": 1, "left-1": -1}.get(mut, 0)
    pos = torch.arange(nq).view(1, nq).expand(H, nq).clone()
    if mut == "first_row_bound":
        pos = torch.zeros_like(pos)
    if mut == "win_pack_pos":                              # packed rows are position-major, row = t * G + g: the bound taken from the row index
        pos = pos * G + (torch.arange(H) % G).view(H, 1)
    shift = n - (t["asked"][b] if mut == "win_nq_unclamped" else nq)
    lb = pos + shift - left
    if mut == "edge_tile_unmasked":
        lb = torch.where(lb > 0, lb // 64 * 64, lb)
    if mut == "edge_tile_skipped":
        lb = torch.where(lb > 0, (lb + 63) // 64 * 64, lb)
    return lb


def win_problem(t, b, mut=None):
    """kvcache_ref.seq_problem with vis AND-ed with the window.  mut: a kvcache_ref mutant (applied to the causal problem) or one of WMUTANTS."""
    c = t["case"]
    assert c["causal"]
    p = K.seq_problem(t, b, mut if mut in K.MUTANTS else None)
    wm = mut if mut in WMUTANTS else None
    n = p["n"]
    j = torch.arange(n).view(1, 1, n)
    p["vis"] = p["vis"] & (j >= left_bounds(t, b, p, wm).unsqueeze(-1))
    if wm == "win_seam" and c["splits"] > 1:               # the last key of every windowed chunk that has a chunk behind it
        for lo, hi in win_chunks(n, p["nq"], c["w"] - 1, c["splits"])[:-1]:
            if lo < hi < n:
                p["vis"][:, :, hi - 1] = False
    return p


def attend_mut(t, b, mut):
    out, lse, _, _ = K.attend(win_problem(t, b, mut))
    return out, lse


def reference(t):
    """Per sequence with rows: b -> (out (nq, H, D), lse (H, nq), A, T, keys of [lo64_b, len_b)) in fp64."""
    w = t["case"]["w"]
    return {b: K.attend(win_problem(t, b)) + (t["lens"][b] - lo64_of(t["lens"][b], t["rows"][b][1], w - 1),) for b in range(t["B"]) if t["rows"][b][1] > 0}


# ---- the emulations: kvcache_ref's, over the windowed chunks ----------------------------------------------------------------------------------------------
def emulate16(t, b, dtype=None):
    """kvcache_ref.emulate16 on the windowed problem: per windowed chunk the 64-key tile loop — P rounded to the 16-bit type against the exact running maximum,
    l summed from the unrounded P —, v_descale on every partial, the merge by the parts' LSEs, ONE rounding of O."""
    dtype = dtype or t["dtype"]
    c = t["case"]
    p = win_problem(t, b)
    H, nq, D = p["q"].shape
    if p["n"] == 0 or nq == 0:
        return torch.zeros(nq, H, D, dtype=torch.float64)
    s = K.scores(p)
    parts = []
    for lo, hi in win_chunks(p["n"], nq, c["w"] - 1, c["splits"]):
        m = torch.full((H, nq, 1), -math.inf, dtype=torch.float64)
        l = torch.zeros(H, nq, 1, dtype=torch.float64)
        o = torch.zeros(H, nq, D, dtype=torch.float64)
        for t0 in range(lo, hi, 64):
            st = s[:, :, t0:min(t0 + 64, hi)]
            mn = torch.maximum(m, st.max(dim=-1, keepdim=True).values)
            safe = torch.where(torch.isfinite(mn), mn, torch.zeros_like(mn))
            alpha = torch.exp(m - safe)
            e = torch.exp(st - safe)
            l = l * alpha + e.sum(-1, keepdim=True)
            o = o * alpha + K.round16(e, dtype) @ p["v"][:, t0:min(t0 + 64, hi)]
            m = mn
        has = l > 0
        ls = torch.where(has, l, torch.ones_like(l))
        parts.append((torch.where(has, o / ls, torch.zeros_like(o)) * p["vd"].view(-1, 1, 1), torch.where(has, m + torch.log(ls), torch.full_like(m, -math.inf))))
    lses = torch.stack([x[1] for x in parts])
    M = lses.max(dim=0).values
    safe = torch.where(torch.isfinite(M), M, torch.zeros_like(M))
    w = torch.exp(lses - safe)
    ws = w.sum(0)
    o = (w * torch.stack([x[0] for x in parts])).sum(0) / torch.where(ws > 0, ws, torch.ones_like(ws))
    return K.round16(o, dtype).transpose(0, 1)


def emulate_lse32(t, b):
    """kvcache_ref.emulate_lse32 on the windowed problem: fp32 throughout, tile by tile over the windowed chunks, tfa_merge's sum over the parts.  (H, nq)."""
    c = t["case"]
    p = win_problem(t, b)
    H, nq, D = p["q"].shape
    f = torch.float32
    if p["n"] == 0 or nq == 0:
        return torch.full((H, nq), math.inf, dtype=f)
    kd = (p["sck"] / t["sc"]).to(f).view(-1, 1, 1)
    sc = torch.tensor(t["sc"] * K.LOG2E, dtype=f) * kd
    sl = torch.tensor(t["sc"], dtype=f) * kd
    raw = torch.einsum("hqd,hkd->hqk", p["q"].to(f), p["k"].to(f)).masked_fill(~p["vis"], -math.inf)
    parts = []
    for lo, hi in win_chunks(p["n"], nq, c["w"] - 1, c["splits"]):
        m = torch.full((H, nq, 1), -1e30, dtype=f)
        l = torch.zeros(H, nq, 1, dtype=f)
        for t0 in range(lo, hi, 64):
            st = raw[:, :, t0:min(t0 + 64, hi)]
            mn = torch.maximum(m, st.max(dim=-1, keepdim=True).values)
            l = l * torch.exp2((m - mn) * sc)
            e = torch.exp2(st * sc - mn * sc)
            for i in range(e.shape[-1]):
                l = l + e[:, :, i:i + 1]
            m = mn
        parts.append(torch.where(l > 0, m * sl + torch.log2(torch.where(l > 0, l, torch.ones_like(l))) * torch.tensor(K.LN2, dtype=f), torch.full_like(l, math.inf)))
    if len(parts) == 1:
        return parts[0].squeeze(-1)
    ls = torch.stack(parts)
    fin = torch.isfinite(ls)
    M = torch.where(fin, ls, torch.full_like(ls, -math.inf)).max(dim=0).values
    w = torch.where(fin, torch.exp(ls - torch.where(torch.isfinite(M), M, torch.zeros_like(M))), torch.zeros_like(ls)).sum(0)
    return torch.where(w > 0, M + torch.log(torch.where(w > 0, w, torch.ones_like(w))), torch.full_like(w, math.inf)).squeeze(-1)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------------------
def edge_keys(c, n, nq):
    """The keys where a window error lives: for the sequence's first and last row the key just outside the window and the first inside it, and the last key of
    every windowed chunk that has a chunk behind it."""
    if n == 0 or nq == 0:
        return []
    left = c["w"] - 1
    hot = set()
    for lb in (n - nq - left, n - 1 - left):
        hot |= {j for j in (lb - 1, lb) if 0 <= j < n}
    if c["splits"] > 1:
        hot |= {hi - 1 for lo, hi in win_chunks(n, nq, left, c["splits"])[:-1] if lo < hi < n}
    return sorted(hot)


def name_wmutants(c):
    """(the window mutants a case can have, [(mutant, why not)]) — structural, as kvcache_ref.name_mutants: which defect has a hot key to act on."""
    rows, asked = K.rows_of(c)
    G = c["H"] // c["Hk"]
    left = c["w"] - 1
    live = [(n, nq, a) for n, (_, nq), a in zip(c["lens"], rows, asked) if nq > 0 and n >= 1]
    edges = [(n, nq, a, lb) for n, nq, a in live for lb in (n - nq - left, n - 1 - left)]
    ok, na = [], []

    def put(m, cond, why):
        ok.append(m) if cond else na.append((m, why))

    put("left+1", any(lb >= 1 for *_, lb in edges), "every window starts at key 0")
    put("left-1", any(lb >= 0 for *_, lb in edges), "every window starts in front of key 0")
    put("edge_tile_unmasked", any(lb >= 1 and lb % 64 for *_, lb in edges), "no edge inside a tile")
    put("edge_tile_skipped", any(lb >= 1 and lb % 64 for *_, lb in edges), "no edge inside a tile")
    put("first_row_bound", any(nq >= 2 and n - 1 - left >= 1 for n, nq, _ in live), "one row per sequence, or the last row's window starts at key 0")
    put("win_pack_pos", K.packs(c) and G > 1 and any(lb >= 0 for *_, lb in edges), "rows not packed, or no window edge at a key")
    put("win_nq_unclamped", c["form"] == "packed" and any(a > nq and n - 1 - left >= 1 for n, nq, a in live), "no nq_b above max_seqlen_q")
    put("win_seam", c["splits"] > 1 and any(sum(1 for lo, hi in win_chunks(n, nq, left, c["splits"]) if lo < hi) > 1 for n, nq, _ in live),
        "one non-empty chunk per sequence (or the library's own split count)")
    return ok, na


def _case(id, w, **kw):
    c = K._case(id, causal=True, **kw)
    assert c["append"] in (None, "4d") and (c["append"] is None or w - 1 >= c["n_new"]), "the window-edge keys must lie in front of the appended rows"
    c["w"] = w
    c["wmutants"], c["wna"] = name_wmutants(c)
    return c


def _packed(id, w, **kw):
    return _case(id, w, form="packed", lq=K.PACKED_LQ, **kw)


def _cases():
    BF16, FP16 = K.BF16, K.FP16
    PL = [128, 700, 1024, 65, 0]
    cs = [
        _case("w4d-bf16-d40-g1-nq1-w1", 1, dtype=BF16, D=40, H=4, Hk=4, Nq=1, lens=[700, 1, 63, 64, 1024], cap=1024, seed=1),
        _case("w4d-fp16-d64-g2-nq5-w2-page64-s2", 2, dtype=FP16, D=64, H=4, Hk=2, Nq=5, lens=[65, 127, 128, 1, 300], cap=512, page=64, splits=2, seed=2),
        _case("w4d-bf16-d104-g4-nq1-w64-page128-s3", 64, dtype=BF16, D=104, H=8, Hk=2, Nq=1, lens=[129, 700, 0, 1024], cap=1024, page=128, splits=3, seed=3),
        _case("w4d-fp16-d128-mqa-nq5-w65-s4-pack", 65, dtype=FP16, D=128, H=8, Hk=1, Nq=5, lens=[300, 64, 1], cap=512, splits=4, pack=True, seed=4),   # <= 3 tiles, 4 chunks
        _case("w4d-bf16-d128-g4-nq130-w100-page256-unpacked", 100, dtype=BF16, D=128, H=8, Hk=2, Nq=130, lens=[700, 129, 1024], cap=1024, page=256, pack=False, seed=5),
        _case("w4d-fp16-d64-g4-nq33-w128-s2-pack", 128, dtype=FP16, D=64, H=8, Hk=2, Nq=33, lens=[300, 65, 512], cap=512, splits=2, pack=True, seed=6),
        _case("w4d-bf16-d64-mqa8-nq1-w512-auto", 512, dtype=BF16, D=64, H=8, Hk=1, Nq=1, lens=[700, 300, 1024], cap=1024, splits=0, seed=7),
        _case("w4d-fp16-d40-g2-nq1-w100-page64-unpacked", 100, dtype=FP16, D=40, H=4, Hk=2, Nq=1, lens=[127, 256, 64], cap=256, page=64, pack=False, seed=8),
        _case("w4d-bf16-d64-g8-nq5-w64-page128-s2", 64, dtype=BF16, D=64, H=8, Hk=1, Nq=5, lens=[700, 129], cap=1024, page=128, splits=2, pack=True, seed=9),
        # fp8 caches
        _case("w4d-fp8-bf16-d48-g2-nq1-w65", 65, dtype=BF16, D=48, H=4, Hk=2, Nq=1, lens=[300, 129], cap=512, fp8=True, seed=20),
        _case("w4d-fp8-fp16-d64-g4-nq5-w128-page128-s3-pack", 128, dtype=FP16, D=64, H=8, Hk=2, Nq=5, lens=[512, 65, 1], cap=512, page=128, splits=3, pack=True,
              fp8=True, seed=21),
        _case("w4d-fp8-bf16-d112-g1-nq1-w64-page64-s2", 64, dtype=BF16, D=112, H=4, Hk=4, Nq=1, lens=[127, 300], cap=512, page=64, splits=2, fp8=True, seed=22),
        _case("w4d-fp8-fp16-d128-mqa-nq5-w2", 2, dtype=FP16, D=128, H=8, Hk=1, Nq=5, lens=[64, 128, 0, 63], cap=256, fp8=True, seed=23),
        # k= / v= in front
        _case("w4d-append-fp16-d104-g1-nq5-w65", 65, dtype=FP16, D=104, H=4, Hk=4, Nq=5, lens=[300, 64, 128], cap=512, append="4d", n_new=5, seed=30),
        _case("w4d-append-fp8-bf16-d64-g2-nq3-w100-page64-s2", 100, dtype=BF16, D=64, H=4, Hk=2, Nq=3, lens=[64, 129], cap=256, page=64, splits=2, fp8=True,
              append="4d", n_new=3, seed=31),
        # packed q (cu_seqlens_q): a length shorter than its nq_b (128 < 300), the capacity, and 0
        _packed("wvq-bf16-d64-g4-w128", 128, dtype=BF16, D=64, H=8, Hk=2, lens=PL, cap=1024, seed=40),
        _packed("wvq-fp16-d128-g2-w100-page128-s3-unpacked", 100, dtype=FP16, D=128, H=4, Hk=2, lens=PL, cap=1024, page=128, splits=3, pack=False, seed=41),
        _packed("wvq-bf16-d40-g1-w512-page64-s2", 512, dtype=BF16, D=40, H=4, Hk=4, lens=PL, cap=1024, page=64, splits=2, seed=42),
        _packed("wvq-fp8-fp16-d112-g2-w65-page256-pack", 65, dtype=FP16, D=112, H=4, Hk=2, lens=PL, cap=1024, page=256, pack=True, fp8=True, seed=43),
        _packed("wvq-bf16-d128-g2-w64-s2-maxq128", 64, dtype=BF16, D=128, H=4, Hk=2, lens=[700, 300, 1024, 65, 0], cap=1024, splits=2, max_q=128, seed=44),
        _packed("wvq-fp16-d64-g2-w2-page64-s4", 2, dtype=FP16, D=64, H=4, Hk=2, lens=PL, cap=1024, page=64, splits=4, seed=45),
    ]
    by = {c["id"]: c for c in cs}
    for base in ("wvq-bf16-d64-g4-w128", "wvq-fp16-d128-g2-w100-page128-s3-unpacked", "wvq-fp8-fp16-d112-g2-w65-page256-pack"):   # the scheduled form: the same result
        cs.append(dict(by[base], id=base + "-sched", sched=True))
    return cs


CASES = _cases()
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES), "case ids must be unique"
SWEEP = 24


def sweep_case(seed):
    """A draw of kvcache_ref.sweep_case (its ranges), made causal, with a window from WINDOWS."""
    c = dict(K.sweep_case(seed), id=f"wsweep{seed}", causal=True)
    c["w"] = random.Random(9000 + seed).choice(WINDOWS)
    c["mutants"], c["na"] = K.name_mutants(c)
    c["wmutants"], c["wna"] = name_wmutants(c)
    return c


def case_of(case_id):
    return BY_ID[case_id] if case_id in BY_ID else sweep_case(int(case_id[len("wsweep"):]))


# ---- the tensors of a case ------------------------------------------------------------------------------------------------------------------------------------
def build(case, dtype=None):
    """kvcache_ref.build's tensors with the window-edge keys (edge_keys) given the weight build gives its hot keys: the same bump along the same direction e
    (the first draw of build's generator; checked against q, whose every row carries ALPHA * e), added to the key where it lies — through the block table,
    re-quantised with the sequence's descale in an fp8 cache, in the cache before an append and in the one behind it (the edge keys lie in front of the
    appended rows: _case asserts it)."""
    c = case
    t = K.build(c, dtype)
    dt = t["dtype"]
    D, Hk = c["D"], c["Hk"]
    g = torch.Generator().manual_seed(1000 + c["seed"])
    e = (torch.randint(0, 2, (D,), generator=g).float() * 2 - 1) / math.sqrt(D)
    assert (t["q"].float() @ e).mean().item() > 0.5 * K.ALPHA, "not build()'s hot direction"
    caches = [t["k_cache"]] + ([t["k_final"]] if t["k_final"] is not t["k_cache"] else [])
    for b, n in enumerate(t["lens"]):
        nq = t["rows"][b][1]
        base = K.hot_keys(c, n)
        bump = max(1.0, math.log(max(n - len(base), 1) / max(len(base), 1)) + 0.5)
        delta = bump / (t["sc"] * K.ALPHA) * e
        for j in edge_keys(c, n, nq):
            if j in base:
                continue
            if c["append"] is not None:
                assert j < int(t["before"][b])
            for cache in caches:
                row = cache[b, j] if t["bt"] is None else cache[int(t["bt"][b, j // c["page"]]), j % c["page"]]      # (Hk, D), a view
                if c["fp8"]:
                    x = (row.float() * t["kd"][b].view(Hk, 1) + delta).to(dt)
                    row.view(torch.uint8).copy_(K.quantise(x, t["kd"][b]).view(torch.uint8))
                else:
                    row.copy_((row.float() + delta).to(dt))
    return t
