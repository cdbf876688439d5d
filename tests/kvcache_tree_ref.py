"""The fp64 definition of flash_attn_with_kvcache(tree_mask=), its per-element bounds, the cases tests/test_kvcache_tree_gpu.py runs on the GPU and
tests/test_kvcache_tree_bounds_cpu.py proves on the CPU, and the tree mutants the bounds must tell from the definition (tests only).

The definition is tests/kvcache_ref.py's — seq_problem / attend, unchanged — with `vis` AND-ed with rule 3 of include/tfa.h (tfa_fwd_kvcache_tree): with
base_b = len_b - nq_b and s = j - base_b, key j is visible to row t iff the causal rule admits it and (s < 0 or s >= 64 or bit s of the row's word is set).
Every case is causal.  The mask removes no tile: chunks, tile counts and so both bounds are kvcache_ref's.  The emulations are kvcache_ref's own functions, run on
the tree problem (patched(): kvcache_ref.seq_problem stands for tree_problem while they run).

Inputs: kvcache_ref.build's, with the keys where a tree goes wrong among its hot keys (tree_keys; patched(): kvcache_ref.hot_keys returns them too while build
runs, so an fp8 cache, an append and a paged pool all see the same keys): for the first, a middle and the last row of every sequence one masked earlier sibling
and one visible ancestor, the last committed key and the first new one, and the new keys on both sides of every tile seam and chunk seam inside the new range.
"""
import contextlib
import random

import torch

import kvcache_ref as K

TMUTANTS = ("bit+1", "bit-1", "row+1", "row_packed", "base_unclamped", "base_seam", "second_tile", "hi_dword", "ge64_masked", "mod64")
KINDS = ("tree", "pattern", "ones")


@contextlib.contextmanager
def patched(**fns):
    """kvcache_ref with some of its functions replaced while the block runs (its file stays as it is)."""
    old = {k: getattr(K, k) for k in fns}
    try:
        for k, f in fns.items():
            setattr(K, k, f)
        yield
    finally:
        for k, f in old.items():
            setattr(K, k, f)


# ---- the masks ----------------------------------------------------------------------------------------------------------------------------------------------
def _signed(w):
    w &= (1 << 64) - 1
    return w - (1 << 64) if w >> 63 else w


def words_of(c):
    """One list of int64 words per sequence, one word per row the sequence ASKS for (packed: lq_b), from the case's seed.
    tree: parent[t] uniform in [-1, t), word[t] = word[parent] | 1 << t for t < 64; rows from the 64th on: all ones, or (long_clear) all ones but one bit below 64.
    pattern: any sub-causal bits; every third row's own bit is clear.  ones: -1.  zero0: the first row's word is 0 (at base_b = 0 the row sees no key)."""
    r = random.Random(5000 + c["seed"])
    _, asked = K.rows_of(c)
    out = []
    for b, a in enumerate(asked):
        ws = []
        for t in range(a):
            if c["mask"] == "ones":
                w = -1
            elif t >= 64:
                w = -1 if not c.get("long_clear") else ~(1 << ((t * 7 + b) % 64))
            elif c["mask"] == "tree":
                par = r.randint(-1, t - 1)
                w = (ws[par] if par >= 0 else 0) | 1 << t
            else:
                w = r.getrandbits(64) & ((1 << (t + 1)) - 1)
                w = w & ~(1 << t) if (b + t) % 3 == 1 else w | 1 << t
            if t == 0 and c.get("zero0") and c["mask"] != "ones":
                w = 0
            ws.append(_signed(w))
        out.append(ws)
    return out


def pack_bool(m):
    """The int64 words of a bool (..., Nq, Nq) mask — what the wrapper computes: sum_s m[..., t, s] << s."""
    nq = m.shape[-1]
    return torch.bitwise_left_shift(m.to(torch.int64), torch.arange(nq, dtype=torch.int64)).sum(dim=-1)


def bool_of(words, nq):
    """The bool (..., nq, nq) form of int64 words (bits at or above nq are dropped: the causal rule never looks at them)."""
    return ((words.unsqueeze(-1) >> torch.arange(nq, dtype=torch.int64)) & 1).bool()


# ---- rule 3, and what a wrong kernel would compute in its place ---------------------------------------------------------------------------------------------
def rule3(c, words, n, nq, asked, mut=None):
    """(H, nq, n) bool: rule 3 for a sequence of n keys and nq rows with `words` ((nq,) int64), by the definition or by a wrong one (TMUTANTS)."""
    H = c["H"]
    G = H // c["Hk"]
    W = words[:nq].view(1, nq).expand(H, nq)
    ones = torch.full((1,), -1, dtype=torch.int64)
    if mut == "row+1":                                     # the word of the next row (the last row: nothing masked)
        W = torch.cat([words[1:nq], ones]).view(1, nq).expand(H, nq)
    if mut == "row_packed":                                # packed rows are position-major, row = t * G + g: the word indexed by the row, not by row / G
        idx = torch.arange(nq).view(1, nq) * G + (torch.arange(H) % G).view(H, 1)
        W = torch.where(idx < nq, words[:nq][idx.clamp(max=max(nq - 1, 0))], ones)
    base = n - (asked if mut == "base_unclamped" else nq)
    s = torch.arange(n) - base
    if mut == "base_seam" and c["splits"] > 1:             # chunk-local key index against a base that was not reduced by the chunk's first key
        for lo, hi in K._chunks(n, c["splits"])[1:]:
            s[lo:hi] -= lo
    if mut == "mod64":
        bi, free = s % 64, torch.zeros(n, dtype=torch.bool)
    else:
        bi, free = s + {"bit+1": 1, "bit-1": -1}.get(mut, 0), (s < 0) | (s >= 64)
    if mut == "ge64_masked":
        free = s < 0
    inr = (bi >= 0) & (bi < 64)
    bit = ((W.unsqueeze(-1) >> bi.clamp(0, 63).view(1, 1, n)) & 1).bool()
    if mut == "hi_dword":                                  # bits 32..63 never looked at
        bit = bit | (bi >= 32).view(1, 1, n)
    vis = free.view(1, 1, n) | ((inr.view(1, 1, n) & bit) if mut == "ge64_masked" else (~inr.view(1, 1, n) | bit))
    if mut == "second_tile":                               # the mask applied in the first 64-key tile the new keys reach only
        vis = vis | (torch.arange(n) // 64 == max(base, 0) // 64 + 1).view(1, 1, n)
    return vis


def tree_problem(t, b, mut=None):
    """kvcache_ref.seq_problem with vis AND-ed with rule 3.  mut: a kvcache_ref mutant (applied to the causal problem) or one of TMUTANTS."""
    c = t["case"]
    assert c["causal"]
    p = _seq_problem(t, b, mut if mut in K.MUTANTS else None)
    q0, nq = t["rows"][b]
    if nq > 0 and p["n"] > 0:
        p["vis"] = p["vis"] & rule3(c, t["words"][q0:q0 + nq], p["n"], nq, t["asked"][b], mut if mut in TMUTANTS else None)
    return p


_seq_problem = K.seq_problem


def attend_mut(t, b, mut):
    out, lse, _, _ = K.attend(tree_problem(t, b, mut))
    return out, lse


def reference(t):
    """Per sequence with rows: b -> (out (nq, H, D), lse (H, nq), A, T, n) in fp64."""
    return {b: K.attend(tree_problem(t, b)) + (t["lens"][b],) for b in range(t["B"]) if t["rows"][b][1] > 0}


def emulate16(t, b, dtype=None):
    """kvcache_ref.emulate16 on the tree problem (per chunk: the mask removes no tile and moves no chunk)."""
    with patched(seq_problem=lambda t_, b_, mut=None: tree_problem(t_, b_)):
        return K.emulate16(t, b, dtype)


def emulate_lse32(t, b):
    """kvcache_ref.emulate_lse32 on the tree problem."""
    with patched(seq_problem=lambda t_, b_, mut=None: tree_problem(t_, b_)):
        return K.emulate_lse32(t, b)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------------------
def tree_keys(c, b, n, words=None):
    """The keys where a tree error lives, for sequence b of n keys: for its first, a middle and its last row the nearest masked earlier sibling and the nearest
    visible ancestor; the last committed key and the first new one; the new keys on both sides of every tile seam and chunk seam inside [base_b, len_b)."""
    rows, _ = K.rows_of(c)
    nq = rows[b][1]
    if n == 0 or nq == 0:
        return []
    ws = (words or words_of(c))[b]
    base = n - nq
    hot = {base - 1, base}
    for r in {0, nq // 2, nq - 1}:
        w = ws[r]
        below = range(min(r, 64) - 1, -1, -1)
        hot |= {base + s for s in next(([s] for s in below if not w >> s & 1), [])}
        hot |= {base + s for s in next(([s] for s in below if w >> s & 1), [])}
    seams = set(range(64, n, 64))
    if c["splits"] > 1:
        seams |= {lo for lo, hi in K._chunks(n, c["splits"])[1:] if lo < n}
    for x in seams:
        if base < x < n:
            hot |= {x - 1, x}
    return sorted(j for j in hot if 0 <= j < n)


def name_tmutants(c):
    """(the tree mutants a case can have, [(mutant, why not)]) — structural: a mutant has something to act on where its rule 3 differs from the definition's at a
    hot key (kvcache_ref.hot_keys or tree_keys) that the causal rule shows to the row."""
    rows, asked = K.rows_of(c)
    words = words_of(c)
    ok, na = [], []
    for m in TMUTANTS:
        hit = False
        for b, (n, (_, nq), a) in enumerate(zip(c["lens"], rows, asked)):
            n = min(max(n, 0), c["cap"])
            if nq == 0 or n == 0:
                continue
            w = torch.tensor(words[b], dtype=torch.int64)
            hot = torch.tensor(sorted(set(K.hot_keys(c, n, tail=False)) | set(tree_keys(c, b, n, words))))
            causal = hot.view(1, -1) <= torch.arange(nq).view(-1, 1) + (n - nq)
            d = (rule3(c, w, n, nq, a) != rule3(c, w, n, nq, a, m))[:, :, hot] & causal.unsqueeze(0)
            hit = hit or bool(d.any())
        ok.append(m) if hit else na.append((m, "its rule 3 is the definition's at every hot key a row sees"))
    return ok, na


def _case(id, mask, **kw):
    c = K._case(id, causal=True, **kw)
    assert mask in KINDS and (c["form"] == "packed" or c["Nq"] <= 64)
    c["mask"] = mask
    c["zero0"], c["long_clear"] = bool(c.pop("zero0", False)), bool(c.pop("long_clear", False))
    c["tmutants"], c["tna"] = name_tmutants(c)
    return c


def _packed(id, mask, **kw):
    return _case(id, mask, form="packed", lq=K.PACKED_LQ, **kw)


def _cases():
    BF16, FP16 = K.BF16, K.FP16
    cs = [
        # 4-D, 16-bit caches: base_b % 64 in {0, 1, 40, 63}, base_b = 0 under a zero word, len_b < Nq, len_b = 0, the capacity
        _case("t4d-bf16-d40-g1-nq40-tree", "tree", dtype=BF16, D=40, H=4, Hk=4, Nq=40, lens=[104, 105, 80, 103, 40], cap=256, zero0=True, seed=1),
        _case("t4d-fp16-d64-g2-nq40-page64-s2", "pattern", dtype=FP16, D=64, H=4, Hk=2, Nq=40, lens=[148, 20, 0, 256], cap=256, page=64, splits=2, seed=2),   # 148: the seam at 128
        _case("t4d-bf16-d104-g4-nq33-page128-s3-pack", "tree", dtype=BF16, D=104, H=8, Hk=2, Nq=33, lens=[200, 97, 512], cap=512, page=128, splits=3, pack=True, seed=3),
        _case("t4d-fp16-d128-mqa8-nq5-auto-unpacked", "pattern", dtype=FP16, D=128, H=8, Hk=1, Nq=5, lens=[68, 5, 300], cap=512, splits=0, pack=False, zero0=True, seed=4),
        _case("t4d-bf16-d64-g8-nq1-page256", "pattern", dtype=BF16, D=64, H=8, Hk=1, Nq=1, lens=[1, 65, 257, 64], cap=512, page=256, seed=5),
        _case("t4d-fp16-d128-g4-nq64-s2-pack", "tree", dtype=FP16, D=128, H=8, Hk=2, Nq=64, lens=[127, 64, 200], cap=256, splits=2, pack=True, seed=6),      # 256 rows: two blocks
        _case("t4d-bf16-d64-g2-nq64-s3", "pattern", dtype=BF16, D=64, H=4, Hk=2, Nq=64, lens=[191, 65, 256], cap=256, splits=3, seed=7),
        # fp8 caches
        _case("t4d-fp8-bf16-d48-g2-nq5", "tree", dtype=BF16, D=48, H=4, Hk=2, Nq=5, lens=[69, 300, 5], cap=512, fp8=True, seed=20),
        _case("t4d-fp8-fp16-d112-g4-nq40-page128-s3-pack", "pattern", dtype=FP16, D=112, H=8, Hk=2, Nq=40, lens=[148, 41, 384], cap=384, page=128, splits=3, pack=True,
              fp8=True, seed=21),
        _case("t4d-fp8-bf16-d64-mqa-nq33-s2", "tree", dtype=BF16, D=64, H=4, Hk=1, Nq=33, lens=[97, 33, 160], cap=256, splits=2, fp8=True, zero0=True, seed=22),
        _case("t4d-fp8-fp16-d128-g1-nq1-page64", "pattern", dtype=FP16, D=128, H=4, Hk=4, Nq=1, lens=[64, 65, 1, 128], cap=256, page=64, fp8=True, seed=23),
        # k= / v= in front: the new keys are the appended rows
        _case("t4d-append-fp16-d104-g1-nq5", "tree", dtype=FP16, D=104, H=4, Hk=4, Nq=5, lens=[300, 68, 128], cap=512, append="4d", n_new=5, seed=30),
        _case("t4d-append-fp8-bf16-d64-g2-nq40-page64-s2", "pattern", dtype=BF16, D=64, H=4, Hk=2, Nq=40, lens=[148, 104], cap=256, page=64, splits=2, fp8=True,
              append="4d", n_new=40, seed=31),
        # packed q (cu_seqlens_q), lq = [300, 1, 130, 0, 64]: rows from the 64th on all ones, or with a cleared bit below 64
        _packed("tvq-bf16-d64-g4-tree", "tree", dtype=BF16, D=64, H=8, Hk=2, lens=[128, 700, 1024, 65, 64], cap=1024, zero0=True, seed=40),
        _packed("tvq-fp16-d128-g2-page128-s3-unpacked-longclear", "tree", dtype=FP16, D=128, H=4, Hk=2, lens=[700, 1, 300, 65, 127], cap=1024, page=128, splits=3,
                pack=False, long_clear=True, seed=41),
        _packed("tvq-bf16-d40-g1-page64-s2-maxq128", "pattern", dtype=BF16, D=40, H=4, Hk=4, lens=[500, 700, 1024, 65, 100], cap=1024, page=64, splits=2, max_q=128,
                long_clear=True, seed=42),
        _packed("tvq-fp8-fp16-d112-g2-page256-pack", "pattern", dtype=FP16, D=112, H=4, Hk=2, lens=[428, 2, 200, 0, 64], cap=1024, page=256, pack=True, fp8=True, seed=43),
        # kvcache_append_varlen (q= rotated in the launch) in front of the packed call
        _packed("tvq-append-bf16-d64-g2-page128-s2", "tree", dtype=BF16, D=64, H=4, Hk=2, lens=[300, 700, 1024, 65, 64], cap=1024, page=128, splits=2, append="varlen",
                long_clear=True, seed=50),
        _packed("tvq-append-fp8-fp16-d48-g2-page64", "pattern", dtype=FP16, D=48, H=4, Hk=2, lens=[300, 700, 1024, 65, 64], cap=1024, page=64, fp8=True, append="varlen",
                seed=51),
    ]
    by = {c["id"]: c for c in cs}
    for base in ("tvq-bf16-d64-g4-tree", "tvq-fp16-d128-g2-page128-s3-unpacked-longclear", "tvq-fp8-fp16-d112-g2-page256-pack"):   # the scheduled form: the same result
        cs.append(dict(by[base], id=base + "-sched", sched=True))
    return cs


CASES = _cases()
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES), "case ids must be unique"
SWEEP = 36


def sweep_case(seed):
    """A draw of kvcache_ref.sweep_case (its ranges), made causal, at most 64 rows in the 4-D form, with a mask kind from the seed."""
    c = dict(K.sweep_case(seed), id=f"tsweep{seed}", causal=True)
    r = random.Random(9500 + seed)
    if c["form"] == "4d":
        c["Nq"] = min(c["Nq"], 64)
    c["mask"], c["zero0"], c["long_clear"] = r.choice(KINDS[:2]), r.random() < 0.3, r.random() < 0.5
    c["mutants"], c["na"] = K.name_mutants(c)
    c["tmutants"], c["tna"] = name_tmutants(c)
    return c


def case_of(case_id):
    return BY_ID[case_id] if case_id in BY_ID else sweep_case(int(case_id[len("tsweep"):]))


# ---- the tensors of a case ------------------------------------------------------------------------------------------------------------------------------------
def build(case, dtype=None):
    """kvcache_ref.build's tensors with tree_keys among the hot keys, and the words: t["words"] (total_q,) int64 — row q0_b + t of sequence b; the 4-D call
    takes them as (B, Nq)."""
    c = case
    words = words_of(c)
    seen = []

    def hot_keys(c_, n, tail=True):
        b = len(seen)
        seen.append(n)
        return sorted(set(_hot_keys(c_, n, tail)) | set(tree_keys(c, b, n, words)))

    with patched(hot_keys=hot_keys):
        t = K.build(c, dtype)
    assert seen == t["lens"], "kvcache_ref.build asks for every sequence's hot keys once, in order"
    t["words"] = torch.tensor([w for ws in words for w in ws], dtype=torch.int64)
    assert t["words"].numel() == t["total_q"]
    return t


_hot_keys = K.hot_keys
