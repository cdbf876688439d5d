"""The fp64 definition of flash_attn_with_kvcache_cascade (include/tfa.h: tfa_fwd_kvcache_cascade), its cases, the fp32 emulation of what runs, the bounds, and the
mutants the bounds must tell from the definition (tests only).  kvcache_ref is imported unchanged: gather, attend, the rounding helpers and both bounds are its own.

The definition, per packed row r: with the header's clamping of both cu arrays, r lies in at most one sequence b (position t = r - q0_b) and at most one group g.
Its keys are the DISJOINT UNION of the group's shared keys [0, plen_g) — all of them, for every row of the group, causal or not — gathered through
prefix_block_table[g], and the sequence's own keys [0, ulen_b) gathered through block_table[b], of which causal leaves j <= t + (ulen_b - nq_b).  out is softmax
attention over the union, lse its logsumexp; a row that sees no key gives out = 0, lse = +inf.  Rows are handled in runs of constant (g, b).

What runs (emulate): level 0 over the shared keys in min(prefix_splits, cap0 / 64) chunks of round_up(ceil(plen_g / ns0), 64) keys and level 1 over the own keys
in min(splits, cap1 / 64) chunks, each chunk the 64-key tile loop of the K/V-cache kernel with its rounding points (kvcache_ref.emulate16 / emulate_lse32) writing
fp32 partials; ONE merge over the ns0 + ns1 parts that skips the empty ones; ONE rounding of O.

Bounds:
  out   kvcache_ref's (B2): eps16 * A + 1e-6 + half an ulp16, A = sum over the UNION of P |v| — the partials and the merge are fp32, O is rounded once.
  lse   kvcache_ref.lse_bound re-derived for ns0 + ns1 parts: every part's LSE carries the one-chunk bound u * [(D + 15) T_p + 4 tiles_p + 13] + 4u |lse_p| with
        T_p <= T (T over the union) and tiles_p <= ceil(max(plen_g, ulen_b) / 64) (no chunk is longer than its level); the merge weights them by w_p / wsum and
        adds u * (5 (ns0 + ns1) + 4) + u |lse| by the same statements as tfa_merge (the skip is a select: no arithmetic of its own).  The merge term is always
        there: this call always merges.  So the bound is lse_bound(T, max(plen_g, ulen_b), lse, D, ns0 + ns1) with ns0 + ns1 >= 2.
"""
import math
import random

import torch

import form_ref as F
import kvcache_ref as K

BF16, FP16 = K.BF16, K.FP16
PAGE = 64
MUTANTS = ("l0_causal", "gb-1", "gb+1", "plen-1", "plen+1", "ushift+1", "ushift-1", "dup", "no_renorm", "scale_empty", "l0_by_seq")


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------------------------
def _case(id, seqs, groups, **kw):
    """seqs: (nq_b, ulen_b) per sequence, packed in order; groups: (sequences in the group, plen_g), the groups cover the first sum(sizes) sequences in order —
    the sequences behind them are in no group; tail: packed rows behind the last sequence, in no sequence and no group; splits: (prefix_splits, splits)."""
    c = dict(id=id, dtype=BF16, H=8, Hk=2, D=64, causal=True, seqs=list(seqs), groups=list(groups), tail=1, splits=(1, 1), pack=None, sched=False, seed=0)
    c.update(kw)
    assert sum(n for n, _ in c["groups"]) <= len(c["seqs"])
    c["mutants"], c["na"] = name_mutants(c)
    return c


def layout(c):
    """rows (q0_b, nq_b) per sequence, grows (r0_g, r1_g) per group, members (the sequences of group g), total_q."""
    rows, q0 = [], 0
    for nq, _ in c["seqs"]:
        rows.append((q0, nq))
        q0 += nq
    grows, members, b = [], [], 0
    for size, _ in c["groups"]:
        members.append(list(range(b, b + size)))
        grows.append((rows[b][0], rows[b + size - 1][0] + rows[b + size - 1][1]))
        b += size
    return rows, grows, members, q0 + c["tail"]


def name_mutants(c):
    """(the mutants the case can have, [(mutant, why not)]) — structural: which defect has something to act on."""
    rows, grows, members, _ = layout(c)
    ok, na = [], []

    def put(m, cond, why):
        ok.append(m) if cond else na.append((m, why))

    plen = [p for _, p in c["groups"]]
    glive = [(g, p) for g, (r0, r1) in enumerate(grows) for p in [plen[g]] if r1 > r0]
    slive = [(nq, u) for nq, u in c["seqs"] if nq > 0]
    both = any(plen[g] >= 1 and c["seqs"][b][0] > 0 and (c["seqs"][b][1] >= c["seqs"][b][0] or not c["causal"]) for g, m in enumerate(members) for b in m)
    put("l0_causal", any(p >= 1 and grows[g][1] - grows[g][0] >= 2 for g, p in glive), "no group with a shared key and two rows")
    inner = [g for g in range(1, len(grows)) if grows[g][0] == grows[g - 1][1] and plen[g] != plen[g - 1]]
    put("gb-1", any(grows[g][0] - 1 >= grows[g - 1][0] and grows[g - 1][1] > grows[g - 1][0] for g in inner), "no boundary between two groups of different shared keys")
    put("gb+1", any(grows[g][1] > grows[g][0] for g in inner), "no boundary between two groups of different shared keys")
    put("plen-1", any(p >= 1 for _, p in glive), "no group with a shared key and a row")
    put("plen+1", bool(glive), "no group with a row")
    put("ushift+1", c["causal"] and any(nq >= 2 and u >= 1 for nq, u in slive), "no causal diagonal below the last row")
    put("ushift-1", c["causal"] and any(u >= 1 and u >= nq for nq, u in slive), "not causal, or no row that sees an own key")
    put("dup", any(p >= 1 for _, p in glive), "no group with a shared key and a row")
    put("no_renorm", both, "no row with keys on both levels")
    one_empty = any(nq > 0 for nq, _ in c["seqs"][sum(n for n, _ in c["groups"]):]) or any(
        c["seqs"][b][0] > 0 and ((plen[g] == 0) != (c["seqs"][b][1] == 0)) for g, m in enumerate(members) for b in m)
    put("scale_empty", one_empty, "no row with keys on exactly one level")
    put("l0_by_seq", any(c["seqs"][b][0] > 0 and plen[min(b, len(plen) - 1)] != plen[g] for g, m in enumerate(members) for b in m), "group index = sequence index")
    return ok, na


# groups of 3 / 1 / 2 sequences and a sequence in no group, a trailing row in nothing; plen in {0, 1, 64, 130}; own lengths from {0, 1, 63, 64, 65, 129}, rows per
# sequence from {0, 1, 5, 33}.  The first group of the "wide" cases has 33 + 5 + 33 = 71 rows: x G = 4 that is 284 packed rows, three query blocks
SEQS_A = [(1, 65), (5, 129), (1, 1), (33, 64), (0, 63), (5, 5), (1, 129)]
SEQS_B = [(33, 129), (5, 65), (33, 33), (1, 0), (5, 63), (1, 64), (5, 129)]
SEQS_C = [(1, 63), (1, 0), (1, 129), (5, 64), (1, 65), (0, 1), (1, 1)]


def _cases():
    cs = []
    n = 0
    for dtype, D in ((BF16, 64), (FP16, 128), (BF16, 128), (FP16, 64)):
        for (H, Hk), pack in (((8, 2), None), ((4, 4), None), ((8, 2), False), ((8, 2), True)):
            if (n // 4 + n) % 2 == 0 and pack is not None:       # half of the pack_gqa variants per (dtype, D): all four splits still meet all three values
                n += 1
                continue
            seqs, plens = ((SEQS_A, (130, 64, 1)), (SEQS_B, (64, 0, 130)), (SEQS_C, (1, 130, 64)), (SEQS_B, (130, 1, 64)))[n % 4]
            splits = ((1, 1), (3, 1), (1, 2), (3, 2))[(n + n // 4) % 4]
            tag = f"{'bf16' if dtype == BF16 else 'fp16'}-d{D}-h{H}k{Hk}-pack{pack}-p{'_'.join(map(str, plens))}-s{splits[0]}{splits[1]}"
            cs.append(_case(f"cs-{tag}", seqs, list(zip((3, 1, 2), plens)), dtype=dtype, D=D, H=H, Hk=Hk, pack=pack, splits=splits, seed=n))
            n += 1
    cs.append(_case("cs-bf16-d64-noncausal-s32", SEQS_A, [(3, 64), (1, 130), (2, 0)], causal=False, splits=(3, 2), seed=40))
    cs.append(_case("cs-fp16-d64-plen0-everywhere", SEQS_C, [(3, 0), (1, 0), (2, 0)], dtype=FP16, splits=(1, 2), seed=41))
    by = {c["id"]: c for c in cs}
    for base in list(by)[:3]:
        cs.append(dict(by[base], id=base + "-sched", sched=True))
    return cs


CASES = _cases()
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES), "case ids must be unique"


def sweep_case(seed):
    r = random.Random(9100 + seed)
    G = r.choice([1, 2, 4])
    Hk = r.choice([1, 2])
    sizes = [r.randint(1, 3) for _ in range(r.randint(1, 3))]
    nseq = sum(sizes) + r.randint(0, 1)
    seqs = [(r.choice([0, 1, 1, 5, 33]), r.choice([0, 1, 63, 64, 65, 129])) for _ in range(nseq)]
    seqs[0] = (max(seqs[0][0], 1), seqs[0][1])
    groups = [(n, r.choice([0, 1, 64, 130])) for n in sizes]
    return _case(f"sweep{seed}", seqs, groups, dtype=r.choice([BF16, FP16]), D=r.choice([64, 128]), H=G * Hk, Hk=Hk, causal=r.random() < 0.8,
                 tail=r.randint(0, 2), splits=(r.randint(1, 3), r.randint(1, 3)), pack=r.choice([None, True, False]), sched=r.random() < 0.3, seed=9100 + seed)


def case_of(case_id):
    return BY_ID[case_id] if case_id in BY_ID else sweep_case(int(case_id[len("sweep"):]))


# ---- the tensors of a case --------------------------------------------------------------------------------------------------------------------------------------
def build(c, nan=False):
    """The tensors of a case on the CPU: q (total_q, H, D); ONE pool k / v (num_pages, 64, Hk, D) behind two shuffled tables bt (B, mb) and pbt (Gn, pmb); cu, lens,
    pcu, plens (int32).  Inputs as kvcache_ref.build: every q row has a component ALPHA along a unit direction e, the hot keys of each level — first, last, first
    behind the length — a bump along e such that they hold about half of a row's weight: one dropped, added, doubled or misplaced key moves out and lse by percents.
    Behind the lengths and in the spare pages: finite garbage (std 1 / 3), or NaN with ``nan`` (what the call must never let through)."""
    dt, H, Hk, D = c["dtype"], c["H"], c["Hk"], c["D"]
    rows, grows, members, total = layout(c)
    B, Gn = len(c["seqs"]), len(c["groups"])
    g = torch.Generator().manual_seed(5000 + c["seed"])
    sc = 1.0 / math.sqrt(D)
    e = (torch.randint(0, 2, (D,), generator=g).float() * 2 - 1) / math.sqrt(D)
    q = (K._randn(g, total, H, D) + K.ALPHA * e).to(dt)
    lens, plens = [u for _, u in c["seqs"]], [p for _, p in c["groups"]]
    mb = max(3, max((u + PAGE) // PAGE for u in lens))                   # every length leaves a key behind it inside the capacity, and three chunks are never clamped
    pmb = max(3, max((p + PAGE) // PAGE for p in plens))
    cap1, cap0 = mb * PAGE, pmb * PAGE
    grp_of = {b: gi for gi, m in enumerate(members) for b in m}

    def keys(n, cap, partner):
        xk, xv = K._randn(g, cap, Hk, D, std=0.5), K._randn(g, cap, Hk, D, std=0.5)
        xk[n:] *= 2.0
        xv[n:] *= 2.0
        hot = sorted({0, n - 1, n} & set(range(cap))) if n else [0]
        cold = n + partner - len(hot)
        bump = max(1.0, math.log(max(cold, 1) / max(len(hot), 1)) + 0.5)
        for j in hot:
            xk[j] += bump / (sc * K.ALPHA) * e
        if nan:
            xk[n:], xv[n:] = math.nan, math.nan
        return xk.to(dt), xv.to(dt)

    own = [keys(u, cap1, plens[grp_of[b]] if b in grp_of else 0) for b, u in enumerate(lens)]
    shared = [keys(p, cap0, max([lens[b] for b in members[gi]])) for gi, p in enumerate(plens)]
    npages = B * mb + Gn * pmb + 3
    perm = torch.randperm(npages, generator=g).to(torch.int32)
    bt, pbt = perm[:B * mb].view(B, mb).contiguous(), perm[B * mb:B * mb + Gn * pmb].view(Gn, pmb).contiguous()
    pools = []
    for i in range(2):
        pool = torch.full((npages, PAGE, Hk, D), math.nan).to(dt) if nan else K._randn(g, npages, PAGE, Hk, D, std=3.0).to(dt)
        for table, src, n in ((bt, own, mb), (pbt, shared, pmb)):
            for r in range(table.shape[0]):
                for j in range(n):
                    pool[int(table[r, j])] = src[r][i][j * PAGE:(j + 1) * PAGE]
        pools.append(pool)
    return dict(case=c, dtype=dt, sc=sc, q=q, k=pools[0], v=pools[1], bt=bt, pbt=pbt, cu=F.cu_of([n for n, _ in c["seqs"]]), lens=torch.tensor(lens, dtype=torch.int32),
                pcu=torch.tensor([r0 for r0, _ in grows] + [grows[-1][1]], dtype=torch.int32), plens=torch.tensor(plens, dtype=torch.int32), total_q=total,
                B=B, Gn=Gn, cap1=cap1, cap0=cap0, max_q=max(1, max(n for n, _ in c["seqs"])), pmax_q=max(1, max(r1 - r0 for r0, r1 in grows)))


def chunks_of(t):
    """(ns0, ns1): the chunk counts the two levels run (tfa.h: min(splits, ceil(capacity / 64)) per level)."""
    ps, s = t["case"]["splits"]
    return min(ps, t["cap0"] // 64), min(s, t["cap1"] // 64)


# ---- the definition ---------------------------------------------------------------------------------------------------------------------------------------------
def clamp_rows(cu, max_q, total):
    """The header's clamp of a cu array: (q0, nq) per entry."""
    res = []
    for i in range(len(cu) - 1):
        c0, c1 = int(cu[i]), int(cu[i + 1])
        q0 = min(max(c0, 0), total)
        res.append((q0, min(max(c1 - c0, 0), min(total - q0, max_q))))
    return res


def runs(t, mut=None):
    """The packed rows in runs of constant (group, sequence): (r0, r1, g or None, b or None); mut moves an inner group boundary by a row."""
    total = t["total_q"]
    pcu = t["pcu"].clone()
    if mut in ("gb-1", "gb+1"):
        pcu[1:-1] += 1 if mut == "gb+1" else -1
    seq, grp = [None] * total, [None] * total
    for arr, cu, mq in ((seq, t["cu"], t["max_q"]), (grp, pcu, t["pmax_q"] + 1)):
        for i, (q0, nq) in enumerate(clamp_rows(cu, mq, total)):
            for r in range(q0, q0 + nq):
                arr[r] = i
    res, r0 = [], 0
    for r in range(1, total + 1):
        if r == total or (grp[r], seq[r]) != (grp[r0], seq[r0]):
            res.append((r0, r, grp[r0], seq[r0], pcu))
            r0 = r
    return res


def problem(t, run, mut=None, level=None):
    """One run of rows as kvcache_ref.attend takes it (keys: the shared ones, then the own ones), and n0, the number of shared keys.  level 0 / 1: that level's keys only."""
    c = t["case"]
    r0, r1, g, b, pcu = run
    H, Hk, D = c["H"], c["Hk"], c["D"]
    nr = r1 - r0
    hk_of = torch.arange(H) // (H // Hk)
    ks, vs, vis = [torch.zeros(0, Hk, D, dtype=torch.float64)], [torch.zeros(0, Hk, D, dtype=torch.float64)], [torch.ones(H, nr, 0, dtype=torch.bool)]
    n0 = 0
    if g is not None and level != 1:
        gi = min(b, t["Gn"] - 1) if (mut == "l0_by_seq" and b is not None) else g
        n0 = int(t["plens"][gi]) + {"plen-1": -1, "plen+1": 1}.get(mut, 0)
        n0 = min(max(n0, 0), t["cap0"])
        k0, v0 = K.gather(t["k"], t["pbt"], gi, n0), K.gather(t["v"], t["pbt"], gi, n0)
        see = torch.ones(H, nr, n0, dtype=torch.bool)
        if mut == "l0_causal":                             # the group taken for a causal sequence of its rows
            g0, nrows = clamp_rows(pcu, t["pmax_q"] + 1, t["total_q"])[g]
            pos = (torch.arange(r0, r1) - g0).view(1, nr, 1)
            see = see & (torch.arange(n0).view(1, 1, n0) <= pos + (n0 - nrows))
        if mut == "dup" and n0:
            k0, v0, see, n0 = torch.cat([k0, k0[-1:]]), torch.cat([v0, v0[-1:]]), torch.cat([see, see[:, :, -1:]], -1), n0 + 1
        ks.append(k0), vs.append(v0), vis.append(see)
    if b is not None and level != 0:
        q0, nq = clamp_rows(t["cu"], t["max_q"], t["total_q"])[b]
        n1 = min(max(int(t["lens"][b]), 0), t["cap1"])
        see = torch.ones(H, nr, n1, dtype=torch.bool)
        if c["causal"]:
            pos = (torch.arange(r0, r1) - q0).view(1, nr, 1)
            see = see & (torch.arange(n1).view(1, 1, n1) <= pos + (n1 - nq) + {"ushift+1": 1, "ushift-1": -1}.get(mut, 0))
        ks.append(K.gather(t["k"], t["bt"], b, n1)), vs.append(K.gather(t["v"], t["bt"], b, n1)), vis.append(see)
    k, v, vis = torch.cat(ks), torch.cat(vs), torch.cat(vis, -1)
    one = torch.ones(H, dtype=torch.float64)
    p = dict(q=t["q"][r0:r1].double().transpose(0, 1), k=k[:, hk_of].transpose(0, 1), v=v[:, hk_of].transpose(0, 1), sck=t["sc"] * one, vd=one, vis=vis,
             n=k.shape[0], nq=nr)
    return p, n0


def reference(t, mut=None):
    """The definition on the whole batch: out (total_q, H, D), lse (H, total_q), A, T in fp64 and n (total_q,) = max(plen_g, ulen_b) of the row (lse_bound's).
    With mut: what a kernel with that defect would give (out, lse only are meaningful)."""
    c = t["case"]
    total, H, D = t["total_q"], c["H"], c["D"]
    out, A = torch.zeros(total, H, D, dtype=torch.float64), torch.zeros(total, H, D, dtype=torch.float64)
    lse, T = torch.full((H, total), math.inf, dtype=torch.float64), torch.zeros(H, total, dtype=torch.float64)
    n = torch.zeros(total, dtype=torch.int64)
    for run in runs(t, mut):
        r0, r1 = run[0], run[1]
        p, n0 = problem(t, run, mut)
        if mut in ("no_renorm", "scale_empty"):
            o0, l0, _, _ = K.attend(problem(t, run, level=0)[0])
            o1, l1, _, _ = K.attend(problem(t, run, level=1)[0])
            live0, live1 = torch.isfinite(l0), torch.isfinite(l1)
            o, l, _, _ = K.attend(p)
            if mut == "no_renorm":                         # the parts summed with weight 1 each instead of exp(lse_p - m)
                cnt = (live0.double() + live1.double()).clamp(min=1.0)
                o = (o0 + o1) / cnt.transpose(0, 1).unsqueeze(-1)
                m = torch.maximum(torch.where(live0, l0, -torch.inf), torch.where(live1, l1, -torch.inf))
                l = torch.where(live0 | live1, m + torch.log(cnt), l)
            else:                                          # 0 x the NaN the workspace held, on every row with exactly one live part
                o = torch.where((live0 != live1).transpose(0, 1).unsqueeze(-1), torch.full_like(o, math.nan), o)
            out[r0:r1], lse[:, r0:r1] = o, l
            continue
        out[r0:r1], lse[:, r0:r1], A[r0:r1], T[:, r0:r1] = K.attend(p)
        n[r0:r1] = max(n0, p["n"] - n0)
    return out, lse, A, T, n


def lse_bound(t, T, n, lse):
    ns0, ns1 = chunks_of(t)
    return K.lse_bound(T, n.view(1, -1), lse, t["case"]["D"], ns0 + ns1)


def ratios(t, out, lse, ref):
    """(max |out - ref| / bound, max |lse - ref| / bound); a NaN, or lse = +inf on other rows than the definition's, counts as infinitely far out."""
    ro, rl, A, T, n = ref
    wo = K.out_ratio(out.double(), ro, A, t["dtype"])
    lse = lse.double()
    if bool(torch.isnan(lse).any()) or not torch.equal(torch.isposinf(lse), torch.isposinf(rl)):
        return wo, math.inf
    fin = torch.isfinite(rl)
    if not bool(fin.any()):
        return wo, 0.0
    b = lse_bound(t, T, n, torch.where(fin, rl, torch.zeros_like(rl)))
    return wo, ((lse - rl).abs()[fin] / b[fin]).max().item()


# ---- what runs, emulated ----------------------------------------------------------------------------------------------------------------------------------------
def _parts16(p, lo0, n, ns, dtype):
    """kvcache_ref.emulate16's chunk loop over the keys [lo0, lo0 + n) of a problem: (O (H, nq, D), lse (H, nq, 1), -inf on an empty part) per chunk."""
    H, nq, D = p["q"].shape
    s = K.scores(p)
    parts = []
    for lo, hi in K._chunks(n, ns):
        m = torch.full((H, nq, 1), -math.inf, dtype=torch.float64)
        l = torch.zeros(H, nq, 1, dtype=torch.float64)
        o = torch.zeros(H, nq, D, dtype=torch.float64)
        for t0 in range(lo, hi, 64):
            sl = slice(lo0 + t0, lo0 + min(t0 + 64, hi))
            st = s[:, :, sl]
            mn = torch.maximum(m, st.max(dim=-1, keepdim=True).values)
            safe = torch.where(torch.isfinite(mn), mn, torch.zeros_like(mn))
            alpha = torch.exp(m - safe)
            e = torch.exp(st - safe)
            l = l * alpha + e.sum(-1, keepdim=True)
            o = o * alpha + K.round16(e, dtype) @ p["v"][:, sl]
            m = mn
        has = l > 0
        ls = torch.where(has, l, torch.ones_like(l))
        parts.append((torch.where(has, o / ls, torch.zeros_like(o)).float().double(), torch.where(has, m + torch.log(ls), torch.full_like(m, -math.inf))))
    return parts


def _lse32(p, lo0, n, ns, sc0):
    """kvcache_ref.emulate_lse32's chunk loop, fp32 throughout: the parts' LSEs (H, nq, 1), +inf on an empty part."""
    H, nq, D = p["q"].shape
    f = torch.float32
    sc, sl = torch.tensor(sc0 * K.LOG2E, dtype=f), torch.tensor(sc0, dtype=f)
    raw = torch.einsum("hqd,hkd->hqk", p["q"].to(f), p["k"].to(f)).masked_fill(~p["vis"], -math.inf)
    parts = []
    for lo, hi in K._chunks(n, ns):
        m = torch.full((H, nq, 1), -1e30, dtype=f)
        l = torch.zeros(H, nq, 1, dtype=f)
        for t0 in range(lo, hi, 64):
            st = raw[:, :, lo0 + t0:lo0 + min(t0 + 64, hi)]
            mn = torch.maximum(m, st.max(dim=-1, keepdim=True).values)
            l = l * torch.exp2((m - mn) * sc)
            e = torch.exp2(st * sc - mn * sc)
            for i in range(e.shape[-1]):
                l = l + e[:, :, i:i + 1]
            m = mn
        parts.append(torch.where(l > 0, m * sl + torch.log2(torch.where(l > 0, l, torch.ones_like(l))) * torch.tensor(K.LN2, dtype=f), torch.full_like(l, math.inf)))
    return parts


def emulate(t):
    """The two partial passes, the skipping merge and the one rounding: out16 (total_q, H, D) as fp64 and lse (H, total_q) fp32."""
    c = t["case"]
    total, H, D = t["total_q"], c["H"], c["D"]
    ns0, ns1 = chunks_of(t)
    out = torch.zeros(total, H, D, dtype=torch.float64)
    lse = torch.full((H, total), math.inf, dtype=torch.float32)
    for run in runs(t):
        r0, r1, g, b, _ = run
        p, n0 = problem(t, run)
        parts, lparts = [], []
        if g is not None:
            parts += _parts16(p, 0, n0, ns0, t["dtype"])
            lparts += _lse32(p, 0, n0, ns0, t["sc"])
        if b is not None:
            parts += _parts16(p, n0, p["n"] - n0, ns1, t["dtype"])
            lparts += _lse32(p, n0, p["n"] - n0, ns1, t["sc"])
        if not parts:
            continue
        # the merge: an empty part is skipped — it takes no part in the maximum, the weights or the sum
        lses = torch.stack([x[1] for x in parts])
        live = torch.isfinite(lses)
        M = lses.max(dim=0).values
        safe = torch.where(torch.isfinite(M), M, torch.zeros_like(M))
        w = torch.where(live, torch.exp(lses - safe), torch.zeros_like(lses))
        acc = torch.where(live, w * torch.stack([x[0] for x in parts]), torch.zeros(1, dtype=torch.float64)).sum(0)
        ws = w.sum(0)
        out[r0:r1] = K.round16(acc / torch.where(ws > 0, ws, torch.ones_like(ws)), t["dtype"]).transpose(0, 1)
        ls = torch.stack(lparts)
        fin = torch.isfinite(ls)
        M = torch.where(fin, ls, torch.full_like(ls, -math.inf)).max(dim=0).values
        w = torch.where(fin, torch.exp(ls - torch.where(torch.isfinite(M), M, torch.zeros_like(M))), torch.zeros_like(ls)).sum(0)
        lse[:, r0:r1] = torch.where(w > 0, M + torch.log(torch.where(w > 0, w, torch.ones_like(w))), torch.full_like(w, math.inf)).squeeze(-1)
    return out, lse


# ---- the equivalent flat problem --------------------------------------------------------------------------------------------------------------------------------
def flat(t):
    """The packed-q call over full per-sequence tables — the group's shared pages prepended to each sequence's own — as a kvcache_ref tensor dict, and the sequences
    on which it is the cascade's definition: the group's plen a page multiple (the flat layout has no room for a partial page), and ulen_b >= nq_b under causal
    (cache_seqlens includes the step's rows: with fewer own keys than rows the flat causal rule would hide shared keys the cascade shows)."""
    c = t["case"]
    rows, grows, members, total = layout(c)
    grp_of = {b: gi for gi, m in enumerate(members) for b in m}
    B, pmb, mb = t["B"], t["pbt"].shape[1], t["bt"].shape[1]
    bt = torch.zeros(B, pmb + mb, dtype=torch.int32)
    lens, same = [], []
    for b in range(B):
        g = grp_of.get(b)
        plen = int(t["plens"][g]) if g is not None else 0
        npg = plen // PAGE
        bt[b, :npg] = t["pbt"][g, :npg] if g is not None else 0
        bt[b, npg:npg + mb] = t["bt"][b]
        lens.append(plen + int(t["lens"][b]))
        same.append(plen % PAGE == 0 and (not c["causal"] or int(t["lens"][b]) >= rows[b][1]))
    fc = dict(H=c["H"], Hk=c["Hk"], D=c["D"], cap=(pmb + mb) * PAGE, causal=c["causal"], splits=1, page=PAGE, form="packed", fp8=False)
    one = torch.ones(B, c["Hk"])
    return dict(case=fc, dtype=t["dtype"], sc=t["sc"], B=B, rows=rows, asked=[n for _, n in rows], lens=lens, q=t["q"], bt=bt, k_final=t["k"], v_final=t["v"],
                kd=one, vd=one, new=None, total_q=total), same
