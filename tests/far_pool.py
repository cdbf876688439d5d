"""A case's K/V caches placed far apart in one arena of 8 GiB + 64 MiB, so that the offsets the K/V-cache family forms — page * page_stride, b * batch_stride, in
elements and in bytes — pass 2^31, 2^32 and 2^33 (tests only; torch only).  tests/test_far_pool_cpu.py proves the placement on a sparse model of the arena,
tests/test_far_pool_gpu.py runs the public calls on it.

The arena is `ARENA_BYTES` of byte 0xFF: NaN as bf16 / fp16 0xFFFF and as e4m3fn.  8 GiB is the least that lets a 16-bit ELEMENT offset pass 2^32; the 64 MiB on
top are 128 of the largest interleaved page among the cases.

Paged caches take the layout an engine uses: the arena viewed as (num_pages, 2, page, Hk, D), k_cache = pool[:, 0], v_cache = pool[:, 1] — one page stride
S = 2 * page * Hk * D elements for both, num_pages = ARENA_BYTES // (S * es), passed to the call as it is.  Every page of the case's small pool (spare and garbage
pages too) moves to a far page index and the block table is rewritten.  The indices, in the order they are handed out: with q(T) = T // (S * es) for T in 2^33,
2^32, 2^31 bytes the pages q(T) + 1 (wholly beyond T whatever the stride), then q(T) (page q starts at T when S * es divides it, and straddles it otherwise:
D 40, 48, 96, 104, 112), then q(T) - 1; the last page; fillers spread between q(2^32) and the end; page 0; fillers in the lower half.  They go first to the pages a live row reads — keys j < len_b of a
sequence with rows, j >= lo64_b under a window —, each sequence's first and last such page in front (kvcache_ref.hot_keys puts its weight there, and an append
writes the last), so that a case with three live pages already has live keys beyond all three thresholds.

The alias rule makes a wrong address loud.  A kernel that truncates an offset to 32 bits would form, for a placed page, one of eight wrong offsets (MUTANTS): the
wrap signed or unsigned, the truncated quantity counted in elements or in bytes, the page base alone or the whole offset truncated.  None of them may land inside
any placed page: a candidate index that would break this, in either direction, is skipped.  A read through a truncated address then returns NaN, a write through
one lands in bytes that must stay 0xFF (Arena.clean).  With power-of-two strides page q(2^32) and page 0 exclude each other: page 0 goes last.

Contiguous caches (B, cap, Hk, D): the arena as (B, 2, cap, Hk, D) through as_strided, batch stride Sb = (arena_elems - 2 * cap * Hk * D) // (B - 1) rounded down
to 16 bytes — the sequences start 2 to 8 GiB apart.  B = 1: the cache sits at the top of the arena, the far offset is in the base pointer alone and no offset the
kernel forms passes a threshold: every mutant is listed as not applicable, with that reason.
"""
import bisect

import torch

import kvcache_ref as K
import kvcache_window_ref as W
import rotary_ref as R

ARENA_BYTES = 2 ** 33 + 2 ** 26
THRESHOLDS = (2 ** 31, 2 ** 32, 2 ** 33)
MUTANTS = tuple((wrap, unit, scope) for wrap in ("s32", "u32") for unit in ("elements", "bytes") for scope in ("page", "whole"))
B1_REASON = "B = 1 contiguous: the offset is in the base pointer"
FP8_NOTE = "fp8: element and byte offsets coincide (the element mutants are the byte mutants)"


def mname(m):
    return "-".join(m)


# ---- the eight truncations -----------------------------------------------------------------------------------------------------------------------------------
def _trunc(x, wrap):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if wrap == "s32" and x >> 31 else x


def wrong_ranges(off, lo, hi, es, m):
    """The byte ranges [(start, length)], relative to the base pointer, that a kernel with truncation m touches for the elements [off + lo, off + hi) of a cache of
    es-byte elements (off: the page / batch base the kernel multiplies out, f * S or b * Sb) — only where they differ from the true ones."""
    wrap, unit, scope = m
    k = es if unit == "bytes" else 1                       # the truncated quantity counts k per element; an address is r of it
    r = es // k
    if hi <= lo:
        return []
    if scope == "page":
        x = off * k
        t = _trunc(x, wrap)
        return [] if t == x else [(t * r + lo * es, (hi - lo) * es)]
    out = []
    a, end = (off + lo) * k, (off + hi) * k
    while a < end:                                         # both wraps are linear between multiples of 2^31
        b = min(end, (a // 2 ** 31 + 1) * 2 ** 31)
        t = _trunc(a, wrap)
        if t != a:
            out.append((t * r, (b - a) * r))
        a = b
    return out


def mutate(off, w, es, m):
    """wrong_ranges for a tensor of element offsets w inside a slot: the byte address (relative to the base pointer) of every element under truncation m (None:
    the true one)."""
    if m is None:
        return (off + w) * es
    wrap, unit, scope = m
    k = es if unit == "bytes" else 1
    r = es // k
    if scope == "page":
        return _trunc(off * k, wrap) * r + w * es
    x = ((off + w) * k) & 0xFFFFFFFF
    if wrap == "s32":
        x = torch.where(x >= 2 ** 31, x - 2 ** 32, x)
    return x * r


# ---- what a case's dict holds --------------------------------------------------------------------------------------------------------------------------------
def layout(t):
    """The parts of a case's dict the placement needs, for kvcache_ref / kvcache_window_ref / kvcache_tree_ref builds, fwd_ref's paged build (k_pool / v_pool) and
    append_varlen_case: the caches in front of the call (kc, vc) and behind it (kf, vf), the table, the geometry, live = [(b, lo, hi)] the key ranges live rows
    read, written = [(b, lo, hi)] the key ranges an append stores."""
    c = t["case"]
    if "k_pool" in t:
        kc, vc = t["k_pool"], t["v_pool"]
        kf, vf, lens, nqs = kc, vc, list(c["lk"]), list(c["lq"])
    else:
        kc, vc, kf, vf, lens, nqs = t["k_cache"], t["v_cache"], t["k_final"], t["v_final"], list(t["lens"]), [r[1] for r in t["rows"]]
    rows, Hk, D = kc.shape[1], kc.shape[2], kc.shape[3]
    live = []
    for b, (n, nq) in enumerate(zip(lens, nqs)):
        if nq > 0 and n > 0:
            live.append((b, W.lo64_of(n, nq, c["w"] - 1) if "w" in c else 0, n))
    written = []
    if t.get("before") is not None:
        written = [(b, int(t["before"][b]), min(lens[b], c["cap"])) for b in range(len(lens)) if min(lens[b], c["cap"]) > int(t["before"][b])]
    return dict(kc=kc, vc=vc, kf=kf, vf=vf, bt=t.get("bt"), es=kc.element_size(), dtype=kc.dtype, rows=rows, Hk=Hk, D=D, half=rows * Hk * D, live=live,
                written=written, B=len(lens))


class Placement:
    """Where a case's slots (pages, or the sequences of a contiguous cache) lie: slot i holds K in the bytes [ptr_k + far[i] * stride * es, + half * es) and V in the
    half * es bytes behind (ptr_v = ptr_k + half * es); the kernel multiplies out far[i] * stride."""

    def __init__(self, L, paged, stride, far, ptr_k, num_pages):
        self.L, self.paged, self.stride, self.far, self.ptr_k, self.num_pages = L, paged, stride, list(far), ptr_k, num_pages
        self.es, self.half = L["es"], L["half"]
        self.slot_bytes = 2 * self.half * self.es
        self.ptr_v = ptr_k + self.half * self.es
        self.bt = None
        if paged:
            self.bt = torch.tensor(self.far, dtype=torch.int64)[L["bt"].long()].to(torch.int32)

    def off(self, i):
        return self.far[i] * self.stride

    def start(self, i):
        return self.ptr_k + self.off(i) * self.es

    def key_slots(self, b, lo, hi):
        """[(slot, first element inside the slot's half, one past the last)] of keys [lo, hi) of sequence b."""
        L = self.L
        hd = L["Hk"] * L["D"]
        if not self.paged:
            return [(b, lo * hd, hi * hd)] if hi > lo else []
        page = L["rows"]
        return [(int(L["bt"][b, i]), (max(lo, i * page) - i * page) * hd, (min(hi, (i + 1) * page) - i * page) * hd) for i in range(lo // page, (hi - 1) // page + 1)
                if hi > lo]

    def changed(self, m, ranges):
        """Whether truncation m changes the address of an element of `ranges` ([(b, lo, hi)] key ranges)."""
        return any(wrong_ranges(self.off(s), a, e, self.es, m) for b, lo, hi in ranges for s, a, e in self.key_slots(b, lo, hi))

    def beyond(self, ranges):
        """{threshold: whether an element of `ranges` lies at or beyond that many bytes of the offset the kernel forms}."""
        top = max([(self.off(s) + e) * self.es for b, lo, hi in ranges for s, a, e in self.key_slots(b, lo, hi)], default=0)
        return {th: top > th for th in THRESHOLDS}

    def wrong_set(self, i):
        return {(p + a, n) for p in (self.ptr_k, self.ptr_v) for m in MUTANTS for a, n in wrong_ranges(self.off(i), 0, self.half, self.es, m)}

    def alias_free(self):
        """The alias rule over the whole placement: no wrong range of any slot meets any slot."""
        starts = sorted(self.start(i) for i in range(len(self.far)))
        return not any(_hits(a, n, starts, self.slot_bytes) for i in range(len(self.far)) for a, n in self.wrong_set(i))

    def mutants(self, ranges=None):
        """(the mutants that change the address of a live key — or of a key of `ranges` —, [(mutant, why not)])."""
        ranges = self.L["live"] if ranges is None else ranges
        ok, na = [], []
        for m in MUTANTS:
            if self.changed(m, ranges):
                ok.append(m)
            elif not self.paged and self.L["B"] == 1:
                na.append((m, B1_REASON))
            elif not ranges:
                na.append((m, "no sequence with a row and a key"))
            else:
                need = 2 ** 32 if m[0] == "u32" else 2 ** 31
                na.append((m, f"no live key at or beyond 2^{need.bit_length() - 1} {m[1]} of the offset"))
        return ok, na


def _hits(a, n, starts, slot_bytes):
    """Whether the byte range [a, a + n) meets one of the disjoint slots [s, s + slot_bytes), s in the sorted list `starts`."""
    i = bisect.bisect_left(starts, a + n) - 1
    return i >= 0 and starts[i] + slot_bytes > a


def _page_order(L):
    """The small pool's pages: each live sequence's first and last live page, the other live pages, the rest."""
    page, bt, seen, order = L["rows"], L["bt"], set(), []

    def put(p):
        if p not in seen:
            seen.add(p)
            order.append(p)

    for b, lo, hi in L["live"]:
        put(int(bt[b, (hi - 1) // page]))
        put(int(bt[b, lo // page]))
    for b, lo, hi in L["live"]:
        for i in range(lo // page, (hi - 1) // page + 1):
            put(int(bt[b, i]))
    for p in range(L["kc"].shape[0]):
        put(p)
    return order


def _candidates(P, num_pages, count):
    qs = [th // P for th in reversed(THRESHOLDS)]
    out = [q + 1 for q in qs] + qs + [q - 1 for q in qs] + [num_pages - 1]
    lo, hi = qs[1] + 2, num_pages - 2
    out += [lo + (i * (hi - lo)) // count for i in range(1, count)]
    out.append(0)
    out += [2 + (i * (qs[2] - 4)) // count for i in range(1, count)]      # below 2^31: only if page 0 was skipped too
    seen = set()
    return [f for f in out if 0 <= f < num_pages and not (f in seen or seen.add(f))]


def place(t):
    """The placement of a case's caches in the arena (a Placement; greedy, see the module's docstring)."""
    L = layout(t)
    es, half = L["es"], L["half"]
    slot = 2 * half
    if L["bt"] is None:
        B = L["B"]
        per16 = 16 // es
        if B == 1:
            top = (ARENA_BYTES // es - slot) // per16 * per16
            return Placement(L, False, slot, [0], top * es, 0)
        Sb = (ARENA_BYTES // es - slot) // (B - 1) // per16 * per16
        return Placement(L, False, Sb, range(B), 0, 0)
    P = slot * es
    num_pages = ARENA_BYTES // P
    nb = L["kc"].shape[0]
    cands = iter(_candidates(P, num_pages, 6 * nb + 32))
    far, starts, wrong = {}, [], set()
    for p in _page_order(L):
        for f in cands:
            mine = {(ptr + a, n) for ptr in (0, half * es) for m in MUTANTS for a, n in wrong_ranges(f * slot, 0, half, es, m)}
            both = sorted(starts + [f * P])
            if any(_hits(a, n, both, P) for a, n in mine) or any(_hits(a, n, [f * P], P) for a, n in wrong):
                continue
            far[p] = f
            bisect.insort(starts, f * P)
            wrong |= mine
            break
        else:
            raise AssertionError(f"{t['case']['id']}: no far page index left for page {p}")
    return Placement(L, True, slot, [far[p] for p in range(nb)], 0, num_pages)


# ---- the sparse model of the arena ---------------------------------------------------------------------------------------------------------------------------
class Sparse:
    """The arena as the placed slots' bytes and 0xFF everywhere else (and outside it: a read there is no read of a key)."""

    def __init__(self, pl, final=False):
        L = pl.L
        self.pl = pl
        n = len(pl.far)
        kc, vc = (L["kf"], L["vf"]) if final else (L["kc"], L["vc"])
        raw = torch.cat([kc.contiguous().view(torch.uint8).reshape(n, -1), vc.contiguous().view(torch.uint8).reshape(n, -1)], dim=1)
        order = sorted(range(n), key=pl.start)
        self.starts = torch.tensor([pl.start(i) for i in order], dtype=torch.int64)
        self.content = raw[order].contiguous().view(-1)

    def read(self, addr):
        """The es bytes at every byte address of `addr` (int64 tensor) -> uint8 (..., es)."""
        pl = self.pl
        a = addr.unsqueeze(-1) + torch.arange(pl.es)
        i = (torch.searchsorted(self.starts, a.contiguous(), right=True) - 1).clamp(min=0)
        rel = a - self.starts[i]
        ok = (rel >= 0) & (rel < pl.slot_bytes) & (a >= 0) & (a < ARENA_BYTES)
        got = self.content[(i * pl.slot_bytes + rel).clamp(0, self.content.numel() - 1)]
        return torch.where(ok, got, torch.full_like(got, 0xFF))

    def gather(self, which, b, lo, hi, m=None):
        """Keys [lo, hi) of sequence b of cache `which` ("k" / "v") as a kernel with truncation m (None: a correct one) reads them: (hi - lo, Hk, D) in the cache's
        dtype."""
        pl, L = self.pl, self.pl.L
        ptr = pl.ptr_k if which == "k" else pl.ptr_v
        parts = [self.read(ptr + mutate(pl.off(s), torch.arange(a, e, dtype=torch.int64), pl.es, m)) for s, a, e in pl.key_slots(b, lo, hi)]
        x = torch.cat(parts) if parts else torch.zeros(0, pl.es, dtype=torch.uint8)
        return x.contiguous().view(-1).view(L["dtype"]).view(hi - lo, L["Hk"], L["D"])


# ---- the arena on the device ---------------------------------------------------------------------------------------------------------------------------------
class Arena:
    """ARENA_BYTES of 0xFF on `dev`, allocated once; put() places a case's caches and returns what the public call takes, take() copies the placed slots out and
    restores them to 0xFF, clean() reads the whole arena once."""

    def __init__(self, dev):
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info(dev)
        if free < ARENA_BYTES + 2 ** 31:
            raise RuntimeError(f"the far-pool arena needs {ARENA_BYTES + 2 ** 31} free bytes on the device (the arena and 2 GiB); {free} are free")
        self.mem = torch.full((ARENA_BYTES,), 0xFF, dtype=torch.uint8, device=dev)

    def _views(self, pl):
        L = pl.L
        if pl.paged:
            pool = self.mem[:pl.num_pages * pl.slot_bytes].view(L["dtype"]).view(pl.num_pages, 2, L["rows"], L["Hk"], L["D"])
            return pool[:, 0], pool[:, 1]
        shape, hd = (L["B"], L["rows"], L["Hk"], L["D"]), L["Hk"] * L["D"]
        flat = self.mem.view(L["dtype"])
        return tuple(flat.as_strided(shape, (pl.stride, hd, L["D"], 1), p // pl.es) for p in (pl.ptr_k, pl.ptr_v))

    def _rows(self, pl):
        return self.mem[:pl.num_pages * pl.slot_bytes].view(pl.num_pages, pl.slot_bytes), torch.tensor(pl.far, dtype=torch.int64, device=self.mem.device)

    def put(self, pl):
        """(k_cache, v_cache, block_table) on the device, the case's caches (as they are in front of the call) in their far slots."""
        L = pl.L
        kv, vv = self._views(pl)
        if pl.paged:
            rows, idx = self._rows(pl)
            n = len(pl.far)
            rows[idx] = torch.cat([L["kc"].contiguous().view(torch.uint8).reshape(n, -1), L["vc"].contiguous().view(torch.uint8).reshape(n, -1)], dim=1).to(self.mem.device)
            return kv, vv, pl.bt.to(self.mem.device)
        kv.copy_(L["kc"].to(self.mem.device))
        vv.copy_(L["vc"].to(self.mem.device))
        return kv, vv, None

    def take(self, pl):
        """The placed slots as the small caches' shapes, on the CPU; the slots are 0xFF again afterwards."""
        L = pl.L
        raw = torch.uint8 if pl.es == 1 else torch.int16
        if pl.paged:
            rows, idx = self._rows(pl)
            got = rows[idx].cpu()
            rows[idx] = 0xFF
            hb = pl.half * pl.es
            return tuple(got[:, a:a + hb].contiguous().view(-1).view(L["dtype"]).view(L["kc"].shape) for a in (0, hb))
        out = []
        for v in self._views(pl):
            out.append(v.contiguous().cpu())
            v.view(raw).fill_(-1 if raw == torch.int16 else 0xFF)
        return tuple(out)

    def clean(self):
        """Whether every byte of the arena is 0xFF: one read of the arena, no temporary."""
        lo, hi = torch.aminmax(self.mem.view(torch.int64))
        return int(lo) == -1 and int(hi) == -1


def same_bits(a, b):
    raw = torch.uint8 if a.element_size() == 1 else torch.int16
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(raw), b.contiguous().view(raw))


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------------------------
SWEEP = 16
# the two k= / v= appends the case lists do not reach: a paged 16-bit one (tfa_kvcache_append, paged) and a contiguous fp8 one (tfa_kvcache_append_fp8, contiguous)
# — kvcache_ref's "4d-append-fp16-d104-g1-nq5-causal" with pages of 128, its "4d-append-fp8-bf16-d64-g2-nq3-causal-page64-s2" without pages
EXTRA = [
    K._case("far-4d-append-fp16-d104-g1-nq5-causal-page128", dtype=K.FP16, D=104, H=4, Hk=4, Nq=5, lens=[300, 64, 128], cap=512, page=128, causal=True, append="4d",
            n_new=5, seed=30),
    K._case("far-4d-append-fp8-bf16-d64-g2-nq3-causal-s2", dtype=K.BF16, D=64, H=4, Hk=2, Nq=3, lens=[64, 129], cap=256, causal=True, splits=2, fp8=True, append="4d",
            n_new=3, seed=31),
]
EXTRA_BY_ID = {c["id"]: c for c in EXTRA}

# kvcache_append_varlen without q= and without fp8 — the plain launch — over tests/test_append_varlen_gpu.py's geometry; a capacity of 192 drops the last
# sequence's rows at positions 192 .. 199
NEW, CACHED, APPEND_HK, APPEND_D = [0, 1, 3, 70], [0, 63, 64, 130], 2, 64
APPEND_VARLEN = ("plain", "neox", "interleaved")


def append_varlen_case(kind, page=64, cap=192):
    """(bf16 into pages, fp16 into a contiguous cache.)  A dict in kvcache_ref.build's form for one plain-launch append: k_new / v_new (total, Hk, D), cu, before, cos / sin (the quarter-turn tables: the rotation is
    exact) and interleaved for the rotary kinds, a shuffled table with three spare pages (page 0: a contiguous cache), garbage of std 3 wherever nothing was
    appended, k_final / v_final as the append is defined to leave them (rows at or beyond the capacity dropped)."""
    assert kind in APPEND_VARLEN
    dtype = K.BF16 if page else K.FP16
    g =torch.Generator().manual_seed(600 + APPEND_VARLEN.index(kind))
    B, Hk, D = len(NEW), APPEND_HK, APPEND_D
    cu = [0]
    for n in NEW:
        cu.append(cu[-1] + n)
    total = cu[-1]
    c = dict(id=f"far-append-varlen-{kind}", page=page, cap=cap, Hk=Hk, D=D, fp8=False, append="plain", B=B, kind=kind)
    kn, vn = (torch.randn(total, Hk, D, generator=g) * 0.5).to(dtype), (torch.randn(total, Hk, D, generator=g) * 0.5).to(dtype)
    cos = sin = None
    kr = kn
    if kind != "plain":
        cos, sin = K.rot_tables(cap + 8, D, dtype)
        pos, valid = R.packed_positions(total, cu, CACHED)
        kr = R.rotary_ref64(kn, cos, sin, pos, kind == "interleaved", valid=valid)[0].to(dtype)
        assert not torch.equal(kr.float(), kn.float())
    mb = cap // page if page else 0
    nb = B * mb + 3 if page else B
    bt = torch.randperm(nb, generator=g)[:B * mb].view(B, mb).to(torch.int32) if page else None
    shape = (nb, page, Hk, D) if page else (B, cap, Hk, D)
    kc, vc = (torch.randn(shape, generator=g) * 3.0).to(dtype), (torch.randn(shape, generator=g) * 3.0).to(dtype)
    kf, vf = kc.clone(), vc.clone()
    for b in range(B):
        for r in range(NEW[b]):
            p = CACHED[b] + r
            if p >= cap:
                continue
            for cache, x in ((kf, kr), (vf, vn)):
                if page:
                    cache[int(bt[b, p // page]), p % page] = x[cu[b] + r]
                else:
                    cache[b, p] = x[cu[b] + r]
    lens = [min(a + n, cap) for a, n in zip(CACHED, NEW)]
    return dict(case=c, dtype=dtype, B=B, k_cache=kc, v_cache=vc, k_final=kf, v_final=vf, bt=bt, lens=lens, rows=[(cu[b], NEW[b]) for b in range(B)],
                before=torch.tensor(CACHED, dtype=torch.int32), cu=torch.tensor(cu, dtype=torch.int32), k_new=kn, v_new=vn, cos=cos, sin=sin)


def modules():
    """{name: (the reference module, its case ids: the list, EXTRA for kvcache_ref, SWEEP seeded draws)}; fwd_ref: its paged cases and its first SWEEP paged draws."""
    import fwd_ref as FR
    import kvcache_tree_ref as T

    paged_draws = []
    seed = 0
    while len(paged_draws) < SWEEP and seed < 2000:
        if FR.sweep_case(seed)["kind"] == "paged":
            paged_draws.append(f"sweep{seed}")
        seed += 1
    assert len(paged_draws) == SWEEP
    return {
        "kvcache": (K, [c["id"] for c in K.CASES] + [c["id"] for c in EXTRA] + [f"sweep{i}" for i in range(SWEEP)]),
        "window": (W, [c["id"] for c in W.CASES] + [f"wsweep{i}" for i in range(SWEEP)]),
        "tree": (T, [c["id"] for c in T.CASES] + [f"tsweep{i}" for i in range(SWEEP)]),
        "prefill": (FR, [c["id"] for c in FR.CASES if c["kind"] == "paged"] + paged_draws),
    }


def case_of(mod, case_id):
    return EXTRA_BY_ID[case_id] if case_id in EXTRA_BY_ID else mod.case_of(case_id)


def families(name, c):
    """The families of the coverage condition a case belongs to."""
    if name == "append_varlen":
        return ["launch tfa_kvcache_append_varlen (plain)"] + (["the contiguous cache"] if not c["page"] else [])
    if name == "prefill":
        return ["paged prefill"]
    fam = [{"kvcache": "the KV-cache forward, fp8" if c["fp8"] else "the KV-cache forward, 16-bit", "window": "windowed", "tree": "tree"}[name]]
    if not c["page"]:
        fam.append("the contiguous cache")
    if c["append"] == "4d":
        fam.append("launch tfa_kvcache_append_fp8" if c["fp8"] else "launch tfa_kvcache_append")
    if c["append"] == "varlen":
        fam.append("launch tfa_kvcache_append_varlen_ex")
    return fam


FAMILIES = ("the KV-cache forward, 16-bit", "the KV-cache forward, fp8", "windowed", "tree", "paged prefill", "the contiguous cache", "launch tfa_kvcache_append",
            "launch tfa_kvcache_append_fp8", "launch tfa_kvcache_append_varlen (plain)", "launch tfa_kvcache_append_varlen_ex")


def record(case_id, pl):
    """The placement of one case as the lines of profiles/far_pool_placement.txt."""
    L = pl.L
    ok, na = pl.mutants()
    far = " ".join(str(f) for f in pl.far)
    geo = (f"pages of {pl.slot_bytes} B, num_pages {pl.num_pages}" if pl.paged else
           f"contiguous, B {L['B']}, batch stride {pl.stride * pl.es} B, base {pl.ptr_k} B")
    lines = [f"{case_id}: {geo}; {len(pl.far)} slots placed", f"    far indices (by small-pool slot): {far}"]
    for what, ranges in (("live keys", L["live"]), ("appended rows", L["written"])):
        if ranges:
            lines.append(f"    {what} beyond " + ", ".join(f"2^{th.bit_length() - 1} B: {'yes' if v else 'no'}" for th, v in pl.beyond(ranges).items()))
    lines.append("    mutants that bite: " + (" ".join(mname(m) for m in ok) or "none"))
    for why in sorted({w for _, w in na}):
        lines.append("    na: " + " ".join(mname(m) for m, w in na if w == why) + f" — {why}")
    if pl.es == 1:
        lines.append(f"    note: {FP8_NOTE}")
    return lines


if __name__ == "__main__":                                 # python tests/far_pool.py > profiles/far_pool_placement.txt
    for name, (mod, ids) in modules().items():
        for cid in ids:
            print("\n".join(record(f"{name}/{cid}", place(mod.build(case_of(mod, cid))))))
    for kind in APPEND_VARLEN:
        for page in (64, 0):
            t = append_varlen_case(kind, page=page)
            print("\n".join(record(f"append_varlen/{t['case']['id']}{'' if page else '-contiguous'}", place(t))))
